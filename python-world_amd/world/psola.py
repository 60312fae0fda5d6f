"""A new f0 contour and a new timing for a recording without analysis and synthesis: time-domain pitch-synchronous
overlap-add (wh_psola, csrc/wh_psola.hip; the contract is in include/world_hip.h, DESIGN section 22, and in NumPy in
tests/_psola_reference.py).

Grains two periods wide are cut around pitch marks of the recording and re-spaced at the target period: the grain spacing
sets f0, the grain content — and with it the spectral envelope — stays.  Where world.tsm.shift_pitch_device moves f0 by
one constant ratio per utterance and the formants with it, this takes a contour and leaves the formants in place.

    y_d, y_off = modify_device(rt, x_d, x_off, fs, enc, pitch=1.25)               # f0 x 1.25, the same duration
    y_d, y_off = modify_device(rt, x_d, x_off, fs, enc, f0=target_f0_d)           # a target f0 per frame of enc
    y_d, y_off = modify_device(rt, x_d, x_off, fs, enc, duration=1.25)            # 1.25 x as long, the same pitch
    y_d, y_off = impose_contour_device(rt, x_d, x_off, fs, enc, times, values)    # set_pitch_contour for a recording

``enc`` is the BatchEncoding or CompactEncoding of the same recordings: its f0 track is where the periods come from.  The
three tracks wh_psola reads (the analysis period, the target period and the source position on a grid of G samples) are
built from the resident tensors with elementwise torch operations — a batch uploads nothing but offsets — and equal what
period_track / source_map compute on the host.

default_params, period_track, source_map, mark_capacity, smark_capacity and check_psola_args are host code and need neither
the library nor a GPU."""
import collections

import numpy as np

from . import _hip
from .tsm import stretched_length

PMAX, MAX_GRID, MAX_HOP, MAX_TOL = 2048, 4096, 2048, 512
Params = collections.namedtuple("Params", "grid hop tol pmin smin norm")


# ---- host ------------------------------------------------------------------------------------------------------------
def default_params(fs, norm=1):
    """Params for a rate: grid 1 ms and unvoiced hop 5 ms in whole samples, tolerance 5 ms (at most 512), pmin =
    floor(fs / 800) (nothing above 800 Hz is a voiced period), smin = max(1, pmin // 2) — (16, 80, 80, 20, 10) at 16 kHz,
    (22, 110, 110, 27, 13) at 22.05 kHz, (48, 240, 240, 60, 30) at 48 kHz."""
    fs = float(fs)
    grid, hop = max(1, int(np.floor(fs * 0.001 + 1e-9))), int(np.floor(fs * 0.005 + 1e-9))
    pmin = int(np.floor(fs / 800.0))
    p = Params(grid, hop, min(MAX_TOL, hop), pmin, max(1, pmin // 2), int(norm))
    check_params(p, "default_params(fs=%r)" % (fs,))
    return p


def check_params(p, where="psola"):
    """ValueError for parameters wh_psola refuses."""
    for name, v, lo, hi in (("grid", p.grid, 1, MAX_GRID), ("hop", p.hop, 1, MAX_HOP), ("tol", p.tol, 0, MAX_TOL),
                            ("pmin", p.pmin, 2, PMAX), ("smin", p.smin, 1, PMAX), ("norm", p.norm, 0, 1)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
            raise ValueError("%s: %s must be an integer in [%d, %d], got %r" % (where, name, lo, hi, v))


def mark_capacity(n, p):
    """ceil(n / m) + 1, m = min(U, pmin - min(tol, pmin // 4)): every analysis step is at least m samples."""
    return -(-int(n) // min(p.hop, p.pmin - min(p.tol, p.pmin // 4))) + 1


def smark_capacity(n_out, p):
    """ceil(n_out / min(U, smin)) + 1."""
    return -(-int(n_out) // min(p.hop, p.smin)) + 1


def _positions(count, grid, time_map, where):
    """float64 [count]: the input sample that grid point k (sample k G) corresponds to.  ``time_map``: None (itself), a
    ratio r of output over input duration (k G / r), or (out_times, in_times), the knots of a piecewise-linear map in
    samples (out_times strictly ascending, at least two; the end segments are extended beyond the ends)."""
    t = np.arange(int(count), dtype=np.float64) * float(grid)
    if time_map is None:
        return t
    if np.ndim(time_map) == 0:
        if not np.isfinite(float(time_map)) or float(time_map) <= 0:
            raise ValueError("%s: the ratio must be positive and finite, got %r" % (where, time_map))
        return t / np.float64(time_map)
    to, ti = (np.asarray(a, dtype=np.float64) for a in time_map)
    if to.ndim != 1 or to.shape != ti.shape or len(to) < 2 or not np.all(np.isfinite(to)) or not np.all(np.isfinite(ti)):
        raise ValueError("%s: a map is two finite 1-D lists of the same length >= 2, got shapes %s and %s" % (where, to.shape, ti.shape))
    if np.any(np.diff(to) <= 0):
        raise ValueError("%s: out_times must ascend strictly" % where)
    seg = np.clip(np.searchsorted(to, t, side="right") - 1, 0, len(to) - 2)
    return ti[seg] + (t - to[seg]) * ((ti[seg + 1] - ti[seg]) / (to[seg + 1] - to[seg]))


def source_map(n_out, grid, time_map=1.0):
    """int64 [n_out // G + 1]: src[k] = floor(c_k + 0.5), c_k the input sample of output sample k G under ``time_map`` (a
    ratio of output over input duration, or (out_times, in_times) in samples)."""
    c = _positions(int(n_out) // int(grid) + 1, grid, time_map, "source_map")
    return np.floor(c + 0.5).astype(np.int64)


def period_track(times, f0, vuv, fs, n, grid, time_map=None, pmin=None):
    """int32 [n // G + 1]: the period in samples at every grid point k G of a signal of n samples.  The grid point's time is
    c_k / fs (c_k = k G, or its image under ``time_map`` when the grid is the OUTPUT's: the target track); the frame is the
    one whose time is nearest, the earlier on a tie; P = floor(fs / f0 + 0.5) where that frame is voiced and f0 > 0, else 0;
    periods outside [pmin, 2048] are 0 (``pmin`` None: floor(fs / 800))."""
    times, f0, vuv = (np.asarray(a, dtype=np.float64) for a in (times, f0, vuv))
    if times.ndim != 1 or times.shape != f0.shape or times.shape != vuv.shape:
        raise ValueError("period_track: times, f0 and vuv must be 1-D and of one length, got %s, %s and %s" % (times.shape, f0.shape, vuv.shape))
    count = int(n) // int(grid) + 1
    if len(times) == 0:
        return np.zeros(count, dtype=np.int32)
    pmin = int(np.floor(float(fs) / 800.0)) if pmin is None else int(pmin)
    t = _positions(count, grid, time_map, "period_track") / np.float64(fs)
    hi = np.clip(np.searchsorted(times, t, side="left"), 0, len(times) - 1)
    lo = np.maximum(hi - 1, 0)
    frame = np.where(t - times[lo] <= times[hi] - t, lo, hi)
    voiced = (vuv[frame] != 0) & (f0[frame] > 0)
    with np.errstate(all="ignore"):
        period = np.floor(np.float64(fs) / np.where(voiced, f0[frame], 1.0) + 0.5)
    ok = voiced & (period >= pmin) & (period <= PMAX)
    return np.where(ok, period, 0.0).astype(np.int32)


def check_psola_args(x_off, y_lengths, p, where="psola"):
    """ValueError for what wh_psola refuses.  Returns (x_off, y_off, pa_off, ps_off, mark_off, smark_off): contiguous int64
    offsets of the recordings, the outputs, the analysis track, the two target tracks, and the mark lists at their
    capacities."""
    check_params(p, where)
    x_off = _hip.check_sample_offsets(x_off, where)
    n = len(x_off) - 1
    if len(y_lengths) != n:
        raise ValueError("%s: %d utterances and %d output lengths" % (where, n, len(y_lengths)))
    lens = _hip.check_output_lengths(y_lengths, where)
    n_in = [int(v) for v in np.diff(x_off)]

    def cum(values):
        return np.concatenate([[0], np.cumsum(values)]).astype(np.int64)

    return (x_off, cum(lens), cum([v // p.grid + 1 for v in n_in]), cum([v // p.grid + 1 for v in lens]),
            cum([mark_capacity(v, p) for v in n_in]), cum([smark_capacity(v, p) for v in lens]))


# ---- device ----------------------------------------------------------------------------------------------------------
def _check_track(rt, t, dtype, count, name, where):
    if t.dim() != 1 or t.dtype != dtype or not t.is_contiguous() or int(t.shape[0]) != count:
        raise ValueError("%s: %s must be a contiguous %s tensor of %d entries" % (where, name, dtype, count))


def psola_device(rt, x_d, x_off, y_lengths, per_a_d, per_s_d, src_d, params, want_marks=False):
    """wh_psola on the resident recordings ``x_d`` (flat, utterance u at x_off[u]:x_off[u+1]) and the three resident tracks
    (int32, int32, int64; utterance u's entries one after the other, n_u // G + 1 of per_a and n_out_u // G + 1 of the
    other two).  Returns (y_d, y_off), and with ``want_marks`` a dict behind them: marks, periods (at mark_off), n_marks,
    smarks, sel, flip (at smark_off), n_smarks — device tensors — and the two host offsets."""
    where = "psola_device"
    x_off, y_off, pa_off, ps_off, mark_off, smark_off = check_psola_args(x_off, y_lengths, params, where)
    torch, n = rt.torch, len(x_off) - 1
    _hip.check_recording(rt, x_d, x_off, where)
    _check_track(rt, per_a_d, torch.int32, int(pa_off[-1]), "per_a", where)
    _check_track(rt, per_s_d, torch.int32, int(ps_off[-1]), "per_s", where)
    _check_track(rt, src_d, torch.int64, int(ps_off[-1]), "src", where)
    with rt.lock, rt.on_stream():
        y_d = rt.empty((int(y_off[-1]),))
        out = None
        if want_marks:
            def z(count, dtype):
                return torch.zeros((int(count),), dtype=dtype, device=rt.device)
            out = {"marks": z(mark_off[-1], torch.int64), "periods": z(mark_off[-1], torch.int32), "n_marks": z(n, torch.int32),
                   "smarks": z(smark_off[-1], torch.int64), "sel": z(smark_off[-1], torch.int32), "flip": z(smark_off[-1], torch.uint8),
                   "n_smarks": z(n, torch.int32)}
        if n:
            opt = [rt.ptr(out[k]) if out else None for k in ("marks", "periods", "n_marks", "smarks", "sel", "flip", "n_smarks")]
            offs = [_hip.i64p(a) for a in (x_off, y_off, pa_off, ps_off, mark_off, smark_off)]
            _hip.check(rt.lib.wh_psola(rt.ctx, rt.stream(), n, *offs, *[int(v) for v in params], rt.ptr(x_d), rt.ptr(per_a_d),
                                       rt.ptr(per_s_d), rt.ptr(src_d), rt.ptr(y_d), *opt))
    if want_marks:
        out["mark_off"], out["smark_off"] = mark_off, smark_off
        return y_d, y_off, out
    return y_d, y_off


def _frame_layout(enc, where):
    fo = getattr(enc, "frame_off", None)
    if fo is None and getattr(enc, "batch", None) is not None:
        fo = enc.batch.frame_off
    if fo is None or getattr(enc, "f0", None) is None or getattr(enc, "vuv", None) is None:
        raise ValueError("%s: enc must be a BatchEncoding or a CompactEncoding, got %r" % (where, type(enc).__name__))
    return np.ascontiguousarray(fo, dtype=np.int64)


def _grid_points(rt, lengths, grid):
    """(utterance of every grid point, k of every grid point) for tracks of length // G + 1 entries, from uploaded counts."""
    torch = rt.torch
    counts = torch.from_numpy(np.asarray([v // grid + 1 for v in lengths], dtype=np.int64)).to(rt.device)
    utt = torch.repeat_interleave(torch.arange(len(lengths), device=rt.device), counts)
    start = torch.cumsum(counts, 0) - counts
    return utt, torch.arange(int(utt.shape[0]), device=rt.device) - start[utt]


def period_track_device(rt, tp_d, f0_d, vuv_d, frame_off, fs, lengths, grid, ratios=None, pmin=None):
    """period_track for every utterance of a batch, on the device: int32, the utterances' tracks one after the other.
    ``ratios`` (one per utterance, output over input duration): the grid is the output's.  Every operation is the host
    function's, in the same order and in float64 — the divisions between tensors, since a division by a host scalar may
    be turned into a product with its reciprocal."""
    torch = rt.torch
    f64 = torch.float64
    n_utt = len(lengths)
    pmin = int(np.floor(float(fs) / 800.0)) if pmin is None else int(pmin)
    utt, k = _grid_points(rt, lengths, grid)
    total = int(utt.shape[0])
    if total == 0 or int(frame_off[-1]) == 0:
        return torch.zeros((total,), dtype=torch.int32, device=rt.device)
    fo = torch.from_numpy(np.ascontiguousarray(frame_off, dtype=np.int64)).to(rt.device)
    fs_t = torch.full((total,), float(fs), dtype=f64, device=rt.device)
    t = k.to(f64) * float(grid)
    if ratios is not None:
        r = torch.from_numpy(np.asarray([float(v) for v in ratios], dtype=np.float64)).to(rt.device)
        t = t / r[utt]
    t = t / fs_t
    first, last = fo[utt], fo[utt + 1]  # this utterance's frames: [first, last)
    empty = last <= first
    # searchsorted(times, t, "left") within [first, last): the first frame whose time is not below t
    lo, hi = first.clone(), last.clone()
    cap = int(tp_d.shape[0]) - 1
    for _ in range(int(np.ceil(np.log2(max(2, int(np.max(np.diff(frame_off))) + 1)))) + 1):
        mid = torch.clamp((lo + hi) // 2, max=cap)
        go = (tp_d[mid] < t) & (lo < hi)
        stay = (~go) & (lo < hi)
        lo = torch.where(go, mid + 1, lo)
        hi = torch.where(stay, mid, hi)
    top = torch.clamp(torch.minimum(lo, last - 1), min=0, max=cap)
    low = torch.clamp(torch.maximum(top - 1, first), max=cap)
    frame = torch.where(t - tp_d[low] <= tp_d[top] - t, low, top)
    voiced = (vuv_d[frame] != 0) & (f0_d[frame] > 0) & ~empty
    period = torch.floor(fs_t / torch.where(voiced, f0_d[frame], torch.ones_like(t)) + 0.5)
    ok = voiced & (period >= pmin) & (period <= PMAX)
    return torch.where(ok, period, torch.zeros_like(period)).to(torch.int32)


def source_map_device(rt, lengths, grid, ratios):
    """source_map for every utterance of a batch (``ratios``: one per utterance), on the device: int64."""
    torch = rt.torch
    utt, k = _grid_points(rt, lengths, grid)
    r = torch.from_numpy(np.asarray([float(v) for v in ratios], dtype=np.float64)).to(rt.device)
    return torch.floor(k.to(torch.float64) * float(grid) / r[utt] + 0.5).to(torch.int64)


def _per_utterance(value, n, name, where):
    v = [value] * n if np.ndim(value) == 0 else list(value)
    if len(v) != n:
        raise ValueError("%s: %d values of %s for %d utterances" % (where, len(v), name, n))
    for r in v:
        if not np.isfinite(float(r)) or float(r) <= 0:
            raise ValueError("%s: %s must be positive and finite, got %r" % (where, name, r))
    return [float(r) for r in v]


def tracks_device(rt, x_off, fs, enc, pitch=1.0, f0=None, duration=1.0, params=None):
    """What modify_device hands to psola_device: (y_lengths, per_a_d, per_s_d, src_d, params)."""
    where = "modify_device"
    params = default_params(fs) if params is None else params
    check_params(params, where)
    torch = rt.torch
    x_off = np.ascontiguousarray(x_off, dtype=np.int64)
    n = len(x_off) - 1
    fo = _frame_layout(enc, where)
    if len(fo) - 1 != n:
        raise ValueError("%s: %d recordings and an encoding of %d utterances" % (where, n, len(fo) - 1))
    ratios = _per_utterance(duration, n, "duration", where)
    n_in = [int(v) for v in np.diff(x_off)]
    n_out = [stretched_length(n_in[u], ratios[u]) for u in range(n)]
    tp_d, f0_d, vuv_d = enc.temporal_positions, enc.f0, enc.vuv
    if not torch.is_tensor(f0_d):
        raise ValueError("%s: the encoding must be resident (a host CompactEncoding: to_device() first)" % where)
    if f0 is None:
        factors = _per_utterance(pitch, n, "pitch", where)
        per_frame = torch.repeat_interleave(torch.from_numpy(np.asarray(factors, dtype=np.float64)).to(rt.device),
                                            torch.from_numpy(np.diff(fo)).to(rt.device))
        target = f0_d * per_frame
    else:
        if not torch.is_tensor(f0) or tuple(f0.shape) != tuple(f0_d.shape) or f0.dtype != torch.float64:
            raise ValueError("%s: f0 must be a float64 device tensor with one value per frame of enc (%d)" % (where, int(f0_d.shape[0])))
        target = f0
    per_a = period_track_device(rt, tp_d, f0_d, vuv_d, fo, fs, n_in, params.grid, None, params.pmin)
    per_s = period_track_device(rt, tp_d, target, vuv_d, fo, fs, n_out, params.grid, ratios, params.pmin)
    return n_out, per_a, per_s, source_map_device(rt, n_out, params.grid, ratios), params


def modify_device(rt, x_d, x_off, fs, enc, pitch=1.0, f0=None, duration=1.0, params=None):
    """The resident recordings with a new pitch and timing.  ``enc``: the BatchEncoding or CompactEncoding of the same
    recordings.  ``pitch``: a factor on f0, or one per utterance; ``f0``: instead, a float64 device tensor with a target f0
    for every frame of enc (a frame is voiced in the target where enc's is and the value is positive): the contour case.
    ``duration``: a ratio of output over input duration, or one per utterance — utterance u becomes round(ratio n_u)
    samples.  ``params``: default_params(fs) when None.  Returns (y_d, y_off).  The formants stay where they are:
    modify_device(.., pitch=world.tsm.log_f0_ratio(a, b)) is the alternative to world.tsm.shift_pitch_device that does not
    move the envelope with f0."""
    with rt.lock, rt.on_stream():
        n_out, per_a, per_s, src, params = tracks_device(rt, x_off, fs, enc, pitch, f0, duration, params)
        return psola_device(rt, x_d, x_off, n_out, per_a, per_s, src, params)


def impose_contour_device(rt, x_d, x_off, fs, enc, times, values=None, params=None):
    """BatchEncoding.set_pitch_contour's counterpart for a recording: the contour (times [s], values [Hz], 0 = unvoiced;
    one pair for every utterance or one per utterance) is interpolated onto enc's frame times with the voiced rule
    (wh_interp_contour) and imposed on the recordings at their own durations.  Returns (y_d, y_off)."""
    from .regrid import interp_contour_device, knot_lists

    fo = _frame_layout(enc, "impose_contour_device")
    off, t, v = knot_lists(times, values, len(fo) - 1, "impose_contour_device")
    with rt.lock, rt.on_stream():
        batch = getattr(enc, "batch", None)
        if batch is None:
            batch = rt.make_batch(np.zeros(len(fo), dtype=np.int64), fo)
        target, _ = interp_contour_device(rt, batch, enc.temporal_positions, off, t, v, True)
        return modify_device(rt, x_d, x_off, fs, enc, f0=target, params=params)


# ---- NumPy forms (World.modify_waveform / World.set_pitch_waveform) ------------------------------------------------------
class _Frames:
    """One utterance's frame tracks on the device, with the two attributes the functions above read of an encoding."""

    def __init__(self, rt, dat, where):
        tp, f0, vuv = (np.ascontiguousarray(dat[k], dtype=np.float64) for k in ("temporal_positions", "f0", "vuv"))
        if tp.ndim != 1 or tp.shape != f0.shape or tp.shape != vuv.shape:
            raise ValueError("%s: temporal_positions, f0 and vuv must be 1-D and of one length" % where)
        self.frame_off = np.array([0, len(tp)], dtype=np.int64)
        self.temporal_positions, self.f0, self.vuv = rt.to_device(tp), rt.to_device(f0), rt.to_device(vuv)


def modify_waveform_numpy(fs, x, dat, pitch=1.0, f0=None, duration=1.0, params=None):
    def run(rt, x_d, x_off):
        enc = _Frames(rt, dat, "modify_waveform")
        target = None if f0 is None else rt.to_device(np.ascontiguousarray(f0, dtype=np.float64))
        return modify_device(rt, x_d, x_off, fs, enc, pitch, target, duration, params)[0]

    return _hip.recording_through("modify_waveform", x, run)


def set_pitch_waveform_numpy(fs, x, dat, time, value, params=None):
    return _hip.recording_through("set_pitch_waveform", x, lambda rt, x_d, x_off: impose_contour_device(
        rt, x_d, x_off, fs, _Frames(rt, dat, "set_pitch_waveform"), time, value, params)[0])
