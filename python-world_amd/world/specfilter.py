"""A per-frame spectral gain applied to an existing waveform (wh_spectral_filter, csrc/wh_specfilter.hip; the contract is
in include/world_hip.h, DESIGN section 19, and in NumPy in tests/_specfilter_reference.py).

The recording is cut into Hanning windows on an integer hop, every window's spectrum is multiplied by the minimum-phase
spectrum of a gain row, and the responses are overlap-added.  The gain is the ratio of two envelopes — two spectrogram
rows, or two rows of line spectral frequencies whose envelopes the kernel evaluates in product form without either of them
in memory — or one envelope alone.  With converted over source envelope this is vocoder-free ("differential") voice
conversion (Kobayashi and Toda): excitation, phase and aperiodicity stay the recording's own and the coding error of the
envelope cancels in the ratio.  The route keeps the source's f0.

    y = filter_device(rt, x_d, batch.x_off, fs, 5, enc.fft_size, num, den)           # any two [F][K] power spectrograms
    y = differential_device(wb, batch, x_d, ce, ce_converted)                         # two encodings of one recording
    y, ce2 = world.gmm.convert_waveform(wb, batch, x_d, ce, model)                    # convert_compact + the filter

default_hop, window_map and check_filter_args are host code and need neither the library nor a GPU."""
import numpy as np

from . import _hip

KINDS = {"spectrum": 0, "lsf": 1}
FFT_SIZES = (512, 1024, 2048, 4096)
MAX_ORDER = 64


# ---- host ------------------------------------------------------------------------------------------------------------
def default_hop(fs, frame_period):
    """The whole samples of a frame period (at least 1), as the Requiem decoder truncates it: 80 at 16 kHz, 110 at
    22.05 kHz (the period is 110.25 samples: window_map keeps the windows on the frame times), 220 at 44.1 kHz and 240
    at 48 kHz, for 5 ms."""
    return max(1, int(np.floor(float(fs) * float(frame_period) / 1000.0 + 1e-9)))


def n_windows(ny, hop):
    """ceil(ny / hop) + 1 windows cover ny samples (window w starts at sample w hop - hop); none for an empty utterance."""
    return 0 if ny <= 0 else -(-int(ny) // int(hop)) + 1


def window_map(ny, n_frames, hop, fs, frame_period):
    """int32 [n_windows]: the frame nearest in time to every window's centre, the 0-based sample w hop - 1:
    min(F - 1, max(0, floor((w hop - 1) * 1000 / (fs * frame_period) + 0.5))), in float64."""
    w = np.arange(n_windows(ny, hop), dtype=np.float64)
    if len(w) and n_frames < 1:
        raise ValueError("window_map: %d samples and no frame" % ny)
    r = np.floor((w * float(hop) - 1.0) * 1000.0 / (float(fs) * float(frame_period)) + 0.5)
    return np.minimum(n_frames - 1, np.maximum(0, r)).astype(np.int32)


_nearest_frame_map = window_map  # (filter_device has a keyword of that name)


def check_filter_args(x_off, frame_off, hops, maps, fft_size, kind, cols_num, cols_den=None, where="filter"):
    """ValueError for what wh_spectral_filter refuses.  ``hops`` / ``maps``: one hop and one int32 list per utterance;
    ``cols_num`` / ``cols_den``: the columns of the gain rows (None: no denominator).  Returns (kind code, p_or_kbins)."""
    if kind not in KINDS:
        raise ValueError("%s: kind must be 'spectrum' or 'lsf', got %r" % (where, kind))
    if isinstance(fft_size, bool) or int(fft_size) != fft_size or int(fft_size) not in FFT_SIZES:
        raise ValueError("%s: fft_size must be a power of two in [512, 4096], got %r" % (where, fft_size))
    k_bins = int(fft_size) // 2 + 1
    if kind == "lsf":
        p = int(cols_num) - 1
        if p < 2 or p > MAX_ORDER or p % 2:
            raise ValueError("%s: rows of line spectral frequencies have an even order in [2, %d], got %d" % (where, MAX_ORDER, p))
        if cols_den is not None and int(cols_den) != int(cols_num):
            raise ValueError("%s: a numerator of order %d against a denominator of order %d" % (where, p, int(cols_den) - 1))
        width = p
    else:
        if int(cols_num) != k_bins or (cols_den is not None and int(cols_den) != k_bins):
            raise ValueError("%s: spectrogram rows must have fft_size / 2 + 1 = %d bins, got %r and %r"
                             % (where, k_bins, cols_num, cols_den))
        width = k_bins
    x_off, frame_off = np.asarray(x_off, dtype=np.int64), np.asarray(frame_off, dtype=np.int64)
    n = len(x_off) - 1
    if n < 0 or len(frame_off) != n + 1 or len(hops) != n or len(maps) != n:
        raise ValueError("%s: %d sample offsets, %d frame offsets, %d hops and %d maps do not describe one batch"
                         % (where, len(x_off), len(frame_off), len(hops), len(maps)))
    if np.any(np.diff(x_off) < 0) or np.any(np.diff(frame_off) < 0) or (n >= 0 and (x_off[0] < 0 or frame_off[0] < 0)):
        raise ValueError("%s: offsets must start at or above 0 and not decrease" % where)
    for u in range(n):
        ny, nf, hop = int(x_off[u + 1] - x_off[u]), int(frame_off[u + 1] - frame_off[u]), hops[u]
        if isinstance(hop, bool) or int(hop) != hop or hop < 1:
            raise ValueError("%s: the hop must be a positive integer, got %r" % (where, hop))
        if 2 * int(hop) - 1 > int(fft_size):
            raise ValueError("%s: a window of 2 * %d - 1 samples is longer than fft_size = %d" % (where, hop, fft_size))
        m = np.asarray(maps[u])
        if m.ndim != 1 or len(m) != n_windows(ny, hop):
            raise ValueError("%s: utterance %d of %d samples at hop %d has %d windows, its map %s entries"
                             % (where, u, ny, hop, n_windows(ny, hop), np.shape(m)))
        if len(m) and (not np.issubdtype(m.dtype, np.integer) or m.min() < 0 or m.max() >= nf):
            raise ValueError("%s: utterance %d: map entries must be integers in [0, %d)" % (where, u, nf))
    return KINDS[kind], width


# ---- device ----------------------------------------------------------------------------------------------------------
def filter_device(rt, x_d, x_off, fs, frame_period, fft_size, num, den=None, kind="spectrum", frame_off=None, hop=None,
                  window_map=None):
    """The waveforms ``x_d`` (flat, utterance u at x_off[u]:x_off[u+1]) filtered window by window: ``y_d`` in x's layout,
    not peak-normalised.  ``num`` / ``den``: [F][K] power spectrograms (kind 'spectrum'), or [F][p + 1] rows
    [log E, cos w_1 .. cos w_p] (kind 'lsf': the COSINES of line spectral frequencies, as world.lsf.envelope_device takes
    them, with the log of the gain in column 0); ``den`` None: ``num`` alone is the gain.  ``frame_off``: the rows of
    every utterance ([0, F] when None: one utterance).  ``hop``: samples between windows (default_hop(fs, frame_period)
    when None; an int, or one per utterance).  ``window_map``: per utterance an int32 list, window -> row of the
    utterance (the frame nearest in time when None)."""
    from .lsf import bin_table

    where = "filter_device"
    x_off = np.ascontiguousarray(x_off, dtype=np.int64)
    n = len(x_off) - 1
    _hip.check_rows(rt, "num", num, where)
    if den is not None:
        _hip.check_rows(rt, "den", den, where)
        if tuple(den.shape) != tuple(num.shape):
            raise ValueError("%s: a numerator %s against a denominator %s" % (where, tuple(num.shape), tuple(den.shape)))
    if frame_off is None:
        frame_off = [0, int(num.shape[0])]
    frame_off = np.ascontiguousarray(frame_off, dtype=np.int64)
    if len(frame_off) != n + 1 or (n >= 0 and int(frame_off[-1]) > int(num.shape[0])):
        raise ValueError("%s: frame offsets %s do not fit %d utterances and %d rows" % (where, frame_off, n, int(num.shape[0])))
    _hip.check_recording(rt, x_d, x_off, where)
    if hop is None:
        hop = default_hop(fs, frame_period)
    hops = [hop] * n if np.ndim(hop) == 0 else list(hop)
    if window_map is None:
        window_map = [_nearest_frame_map(int(x_off[u + 1] - x_off[u]), int(frame_off[u + 1] - frame_off[u]), hops[u], fs, frame_period)
                      if float(hops[u]) >= 1 else np.zeros(0, dtype=np.int32) for u in range(min(n, len(hops)))]
    code, width = check_filter_args(x_off, frame_off, hops, window_map, fft_size, kind, int(num.shape[1]),
                                    None if den is None else int(den.shape[1]), where)
    maps = [np.asarray(m, dtype=np.int32) for m in window_map]
    map_off = np.concatenate([[0], np.cumsum([len(m) for m in maps])]).astype(np.int64)
    h_map = np.ascontiguousarray(np.concatenate(maps) if maps else np.zeros(0), dtype=np.int32)
    h_hop = np.ascontiguousarray(hops, dtype=np.int64)
    ctab = bin_table(int(fft_size) // 2 + 1) if kind == "lsf" else None
    with rt.lock, rt.on_stream():
        y_d = rt.empty((int(x_d.shape[0]),))
        if int(x_d.shape[0]) > int(x_off[-1]) or (n and int(x_off[0]) > 0):
            y_d.zero_()  # (samples outside every utterance)
        _hip.check(rt.lib.wh_spectral_filter(
            rt.ctx, rt.stream(), n, _hip.i64p(x_off), _hip.i64p(frame_off), _hip.i64p(map_off), _hip.i32p(h_map),
            _hip.i64p(h_hop), code, rt.ptr(num), _hip.ld(num), rt.ptr(den), _hip.ld(den) if den is not None else 0, width,
            _hip.f64p(ctab) if ctab is not None else None, int(fft_size), rt.ptr(x_d), rt.ptr(y_d)))
    return y_d


def _lsf_cosine_rows(rt, rows):
    """[log E, w_1 .. w_p] (radians) -> [log E, cos w_1 .. cos w_p]: what the kernel takes."""
    torch = rt.torch
    out = rt.empty(tuple(rows.shape))
    out[:, 0] = rows[:, 0]
    torch.cos(rows[:, 1:], out=out[:, 1:])
    return out


def _describe(e):
    from .batch import BatchEncoding
    from .compact import CompactEncoding

    if isinstance(e, BatchEncoding):
        return ("batch", None, e.fs, int(e.fft_size), int(e.spectrogram.shape[0]))
    if isinstance(e, CompactEncoding):
        if e.kind == "spectrogram":
            raise ValueError("differential_device: a CompactEncoding that keeps the dense spectrogram: hand in the BatchEncoding")
        return (e.kind, e.lsf_order if e.kind == "lsf" else e.n0, e.fs, int(e.fft_size), e.total_frames)
    raise ValueError("differential_device: source and target are BatchEncodings or CompactEncodings, got %r" % type(e).__name__)


def differential_device(wb, batch, x_d, source, target, hop=None, window_map=None):
    """The recording ``x_d`` of ``batch`` (WorldBatch.upload's pair) filtered by target over source envelope: y_d in x's
    layout.  ``source`` and ``target`` are two encodings of the same frames: two BatchEncodings (their spectrograms), two
    CompactEncodings of line spectral frequencies (the rows directly: the kernel forms both envelopes per bin) or two of
    mel-cepstra (their expanded spectrograms).  ValueError on mismatched kinds, rates, orders or frame counts."""
    ds, dt = _describe(source), _describe(target)
    if ds != dt:
        raise ValueError("differential_device: source (kind %r, order %r, fs %r, fft_size %d, %d frames) against target "
                         "(kind %r, order %r, fs %r, fft_size %d, %d frames)" % (ds + dt))
    kind, _, fs, fft_size, frames = ds
    if frames != batch.total_frames:
        raise ValueError("differential_device: encodings of %d frames against a batch of %d" % (frames, batch.total_frames))
    frame_period = getattr(batch, "frame_period", None) or source.frame_period
    if frame_period is None:
        raise ValueError("differential_device: neither the batch nor the source encoding knows its frame period")
    rt = wb.rt
    with rt.lock, rt.on_stream():
        if kind == "batch":
            num, den, fkind = target.spectrogram, source.spectrogram, "spectrum"
        elif kind == "lsf":
            s, t = source.to_device(rt), target.to_device(rt)
            num, den, fkind = _lsf_cosine_rows(rt, t.lsf), _lsf_cosine_rows(rt, s.lsf), "lsf"
        else:
            num, den, fkind = target.expand(wb).spectrogram, source.expand(wb).spectrogram, "spectrum"
        return filter_device(rt, x_d, batch.x_off, fs, frame_period, fft_size, num, den, fkind, batch.frame_off, hop,
                             window_map)


# ---- NumPy form (World.filter_waveform) --------------------------------------------------------------------------------
@_hip.serialised
def filter_waveform_numpy(fs, x, dat_num, dat_den=None):
    """x filtered by dat_num's spectrogram over dat_den's (encode() dicts of the same frame grid; dat_den None: by
    dat_num's alone): a NumPy array like x."""
    x = _hip.host_recording(x, "filter_waveform")
    sn = np.asarray(dat_num['spectrogram'], dtype=np.float64)
    sd = None if dat_den is None else np.asarray(dat_den['spectrogram'], dtype=np.float64)
    if sn.ndim != 2 or (sd is not None and sd.shape != sn.shape):
        raise ValueError("filter_waveform: spectrograms of shape %s and %s" % (sn.shape, None if sd is None else sd.shape))
    if dat_num['fs'] != fs or (dat_den is not None and dat_den['fs'] != fs):
        raise ValueError("filter_waveform: the dicts were encoded at another sampling rate than fs = %r" % (fs,))
    tp = np.asarray(dat_num['temporal_positions'], dtype=np.float64)
    frame_period = float(tp[1] - tp[0]) * 1000.0 if len(tp) > 1 else 5.0
    frame_period = round(frame_period * 1e6) / 1e6
    fft_size = 2 * (sn.shape[0] - 1)
    rt = _hip.Runtime.get()
    with rt.lock, rt.on_stream():
        num = rt.to_device(sn).transpose(0, 1).contiguous()
        den = None if sd is None else rt.to_device(sd).transpose(0, 1).contiguous()
        y = filter_device(rt, rt.to_device(x), [0, len(x)], fs, frame_period, fft_size, num, den)
        out = y.cpu().numpy()
    rt.check_flags("filter_waveform")
    return out
