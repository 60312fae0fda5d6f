"""Mel-cepstra with a first-order all-pass warp, the SPTK convention, at any sampling rate (the contract
is in NumPy in tests/_melcep_reference.py).

Rows c[0 .. m] code a POWER spectrum row on the axis beta(w) = w + 2 atan2(alpha sin w, 1 - alpha cos w):
log P[k] = 2 sum_j c[j] cos(j beta_k), beta_k = beta(pi k / (K - 1)).  Coding is SPTK's ``freqt`` of the cepstrum of
log P and is linear in log P, decoding is a cosine sum: each is ONE host-built table through the product kernel
(wh_feature_matmul_tagged: the logarithm as its prologue, the exponential as its epilogue).  A recording is filtered by a
difference of two rows in closed form (wh_melcep_filter: exp(sum_j d[j] z~^-j) is minimum phase as it stands), so neither
envelope is ever in memory.

    mc = melcep_device(rt, enc.spectrogram, 24, default_alpha(fs))            # [F][25], order 24 at 16 kHz
    sp = spectrum_device(rt, mc, enc.fft_size, default_alpha(fs))             # [F][K]
    db = mcd_db_device(mc_a, mc_b)                                            # [F] mel-cepstral distortion
    y = differential_device(wb, batch, x_d, mc_source, mc_converted, fs, enc.fft_size)

The rows are plain [F][m + 1] tensors: delta_features_device, mlpg_device, align_device, gmm.fit_device / convert_device
and wh_knn take them as they are.  The tables and the argument checks are host code and need neither the library nor a GPU."""
import functools

import numpy as np

from . import _hip
from . import specfilter as _sf
from .features import _Tagged, feature_matmul_device

MAX_ORDER = 64
MCD_SCALE = 10.0 / np.log(10.0)
# the customary warps per sampling rate (they are conventions, not fits: a least-squares fit of beta to the mel scale
# gives 0.459 at 16 kHz)
DEFAULT_ALPHA = {8000: 0.31, 10000: 0.35, 12000: 0.37, 16000: 0.42, 22050: 0.45, 24000: 0.466, 32000: 0.504, 44100: 0.544,
                 48000: 0.554}


# ---- host ------------------------------------------------------------------------------------------------------------
def default_alpha(fs):
    """The customary all-pass constant of the sampling rate ``fs``; ValueError for a rate without one."""
    if isinstance(fs, bool) or int(fs) != fs or int(fs) not in DEFAULT_ALPHA:
        raise ValueError("melcep: no customary alpha for fs = %r (%s): pass alpha" % (fs, sorted(DEFAULT_ALPHA)))
    return DEFAULT_ALPHA[int(fs)]


def _alpha(alpha, fs, where):
    if alpha is None and fs is None:
        raise ValueError("%s: alpha is needed (default_alpha(fs) has the customary ones)" % where)
    alpha = default_alpha(fs) if alpha is None else float(alpha)
    if not -1.0 < alpha < 1.0:
        raise ValueError("%s: alpha must lie inside (-1, 1), got %r" % (where, alpha))
    return alpha


def check_order(order, where="melcep", k_bins=None):
    if isinstance(order, bool) or int(order) != order or order < 1 or order > MAX_ORDER:
        raise ValueError("%s: the order must be an integer in [1, %d], got %r" % (where, MAX_ORDER, order))
    if k_bins is not None and (k_bins < 3 or int(order) > k_bins - 1):
        raise ValueError("%s: %d bins are too few for order %d" % (where, k_bins, order))
    return int(order)


def _beta(k_bins, alpha):
    w = np.pi * np.arange(k_bins) / (k_bins - 1)
    return w + 2 * np.arctan2(alpha * np.sin(w), 1 - alpha * np.cos(w))


@functools.lru_cache(maxsize=16)
def warp_tables(k_bins, alpha):
    """(cos beta_k, sin beta_k), k < K: the warped axis as wh_melcep_filter takes it.  The ends are exact."""
    b = _beta(int(k_bins), float(alpha))
    c, s = np.cos(b), np.sin(b)
    c[0], c[-1], s[0], s[-1] = 1.0, -1.0, 0.0, 0.0
    c.setflags(write=False)
    s.setflags(write=False)
    return c, s


def _freqt_matrix(n_in, order, alpha):
    """[order + 1][n_in]: SPTK's freqt as a matrix (the recursion run on the unit sequences, all at once)."""
    g = np.zeros((order + 1, n_in))
    unit = np.eye(n_in)
    for i in range(n_in - 1, -1, -1):
        d = g.copy()
        g[0] = unit[i] + alpha * d[0]
        g[1] = (1 - alpha * alpha) * d[0] + alpha * d[1]
        for j in range(2, order + 1):
            g[j] = d[j - 1] + alpha * (d[j] - g[j - 1])
    return g


@functools.lru_cache(maxsize=16)
def encode_table(k_bins, order, alpha):
    """[K][m + 1]: log P row -> c.  q = irfft(log P)[0 .. N/2] with q[0] and q[N/2] halved, then freqt: column j is the
    cosine transform of freqt's row j, taken as the real transform of its even extension."""
    k_bins, order, alpha = int(k_bins), int(order), float(alpha)
    n = 2 * (k_bins - 1)
    a = _freqt_matrix(k_bins, order, alpha)                    # c = a q
    even = np.concatenate([a, a[:, -2:0:-1]], axis=1)          # sum_n h_n a[n] cos(2 pi k n / N) = rfft(even)[k] / 2
    w = np.full(k_bins, 2.0)
    w[0] = w[-1] = 1.0
    return _Tagged((np.fft.rfft(even, axis=1).real * (0.5 * w / n)[None, :]).T)


@functools.lru_cache(maxsize=16)
def decode_table(order, alpha, k_bins):
    """[m + 1][K] = 2 cos(j beta_k): c -> log P row."""
    j = np.arange(int(order) + 1, dtype=np.float64)[:, None]
    return _Tagged(2.0 * np.cos(j * _beta(int(k_bins), float(alpha))[None, :]))


# ---- device ----------------------------------------------------------------------------------------------------------
def melcep_device(rt, spec_d, order, alpha):
    """Mel-cepstra [F][order + 1] of a POWER spectrogram [F][K] (BatchEncoding.spectrogram is one)."""
    _hip.check_rows(rt, "spec", spec_d, "melcep", 3)
    f, k_bins = (int(v) for v in spec_d.shape)
    order, alpha = check_order(order, "melcep", k_bins), _alpha(alpha, None, "melcep")
    return feature_matmul_device(rt, spec_d, f, k_bins, _hip.ld(spec_d), encode_table(k_bins, order, alpha), prologue=2)


def spectrum_device(rt, rows_d, fft_size, alpha):
    """The POWER spectrogram [F][fft_size / 2 + 1] that the rows [F][m + 1] code."""
    _hip.check_rows(rt, "rows", rows_d, "spectrum", 2)
    if isinstance(fft_size, bool) or int(fft_size) != fft_size or fft_size < 4 or int(fft_size) % 2:
        raise ValueError("spectrum: fft_size must be an even integer of at least 4, got %r" % (fft_size,))
    f, cols = (int(v) for v in rows_d.shape)
    k_bins = int(fft_size) // 2 + 1
    order, alpha = check_order(cols - 1, "spectrum"), _alpha(alpha, None, "spectrum")
    return feature_matmul_device(rt, rows_d, f, cols, _hip.ld(rows_d), decode_table(order, alpha, k_bins), epilogue=2)


def mcd_db_device(rows_a, rows_b):
    """[F]: the mel-cepstral distortion in dB of every pair of rows, (10 / ln 10) sqrt(2 sum_{j >= 1} (a[j] - b[j])^2)."""
    if rows_a.dim() != 2 or tuple(rows_a.shape) != tuple(rows_b.shape) or int(rows_a.shape[1]) < 2:
        raise ValueError("mcd_db: rows of shape %s against %s" % (tuple(rows_a.shape), tuple(rows_b.shape)))
    d = rows_a[:, 1:] - rows_b[:, 1:]
    return MCD_SCALE * (2.0 * (d * d).sum(dim=1)).sqrt()


def filter_device(rt, x_d, x_off, fs, frame_period, fft_size, num, den=None, alpha=None, frame_off=None, hop=None,
                  window_map=None):
    """world.specfilter.filter_device with mel-cepstral gain rows: ``num`` / ``den`` are [F][m + 1] rows of one order and
    one ``alpha`` (default_alpha(fs) when None); ``den`` None: ``num`` alone is the gain.  The geometry (hop, windows,
    row map, frame offsets) is the spectral filter's, argument for argument."""
    where = "melcep.filter_device"
    x_off = np.ascontiguousarray(x_off, dtype=np.int64)
    n = len(x_off) - 1
    _hip.check_rows(rt, "num", num, where)
    if den is not None:
        _hip.check_rows(rt, "den", den, where)
        if tuple(den.shape) != tuple(num.shape):
            raise ValueError("%s: a numerator %s against a denominator %s" % (where, tuple(num.shape), tuple(den.shape)))
    order = check_order(int(num.shape[1]) - 1, where)
    alpha = _alpha(alpha, fs, where)
    if frame_off is None:
        frame_off = [0, int(num.shape[0])]
    frame_off = np.ascontiguousarray(frame_off, dtype=np.int64)
    if len(frame_off) != n + 1 or (n >= 0 and int(frame_off[-1]) > int(num.shape[0])):
        raise ValueError("%s: frame offsets %s do not fit %d utterances and %d rows" % (where, frame_off, n, int(num.shape[0])))
    _hip.check_recording(rt, x_d, x_off, where)
    if hop is None:
        hop = _sf.default_hop(fs, frame_period)
    hops = [hop] * n if np.ndim(hop) == 0 else list(hop)
    if window_map is None:
        window_map = [_sf.window_map(int(x_off[u + 1] - x_off[u]), int(frame_off[u + 1] - frame_off[u]), hops[u], fs, frame_period)
                      if float(hops[u]) >= 1 else np.zeros(0, dtype=np.int32) for u in range(min(n, len(hops)))]
    # (the geometry checks do not depend on the kind: they are asked for with rows of fft_size / 2 + 1 columns)
    k_bins = int(fft_size) // 2 + 1 if not isinstance(fft_size, bool) and int(fft_size) == fft_size else 0
    _sf.check_filter_args(x_off, frame_off, hops, window_map, fft_size, "spectrum", k_bins, None, where)
    maps = [np.asarray(m, dtype=np.int32) for m in window_map]
    map_off = np.concatenate([[0], np.cumsum([len(m) for m in maps])]).astype(np.int64)
    h_map = np.ascontiguousarray(np.concatenate(maps) if maps else np.zeros(0), dtype=np.int32)
    h_hop = np.ascontiguousarray(hops, dtype=np.int64)
    cos_b, sin_b = warp_tables(k_bins, alpha)
    with rt.lock, rt.on_stream():
        y_d = rt.empty((int(x_d.shape[0]),))
        if int(x_d.shape[0]) > int(x_off[-1]) or (n and int(x_off[0]) > 0):
            y_d.zero_()  # (samples outside every utterance)
        _hip.check(rt.lib.wh_melcep_filter(
            rt.ctx, rt.stream(), n, _hip.i64p(x_off), _hip.i64p(frame_off), _hip.i64p(map_off), _hip.i32p(h_map),
            _hip.i64p(h_hop), rt.ptr(num), _hip.ld(num), rt.ptr(den), _hip.ld(den) if den is not None else 0, order,
            _hip.f64p(cos_b), _hip.f64p(sin_b), int(fft_size), rt.ptr(x_d), rt.ptr(y_d)))
    return y_d


def differential_device(wb, batch, x_d, rows_source, rows_target, fs, fft_size, alpha=None, hop=None, window_map=None):
    """The recording ``x_d`` of ``batch`` (WorldBatch.upload's pair) filtered by target over source envelope, both given
    as mel-cepstral rows [total frames][m + 1] on the batch's frame grid: y_d in x's layout.  Vocoder-free conversion as
    Kobayashi and Toda describe it, on the code they describe it on."""
    if int(rows_source.shape[0]) != batch.total_frames:
        raise ValueError("melcep.differential_device: rows of %d frames against a batch of %d"
                         % (int(rows_source.shape[0]), batch.total_frames))
    frame_period = getattr(batch, "frame_period", None)
    if frame_period is None:
        raise ValueError("melcep.differential_device: the batch does not know its frame period")
    return filter_device(wb.rt, x_d, batch.x_off, fs, frame_period, fft_size, rows_target, rows_source, alpha, batch.frame_off,
                         hop, window_map)


# ---- NumPy forms (World.encode_melcep / decode_melcep / melcep_distortion / filter_waveform_melcep) --------------------
@_hip.serialised
def _on_device(fn, x, *a, **kw):
    rt = _hip.Runtime.get()
    out = fn(rt, rt.to_device(np.ascontiguousarray(x, dtype=np.float64)), *a, **kw)
    rt.check_flags(fn.__name__)
    return out.cpu().numpy()


def _check_host_rows(x, where, min_cols):
    if np.ndim(x) != 2 or np.shape(x)[1] < min_cols:
        raise ValueError("%s: expected (N frames, >= %d columns), got shape %s" % (where, min_cols, np.shape(x)))


def encode_melcep(spec, order=24, alpha=None, fs=16000):
    """(N, D) POWER spectrogram (encode()'s 'spectrogram', transposed) -> (N, order + 1) mel-cepstra."""
    _check_host_rows(spec, "encode_melcep", 3)
    check_order(order, "encode_melcep", np.shape(spec)[1])
    return _on_device(melcep_device, spec, int(order), _alpha(alpha, fs, "encode_melcep"))


def decode_melcep(mc, fft_size, alpha=None, fs=16000):
    """(N, m + 1) mel-cepstra -> the (N, fft_size / 2 + 1) POWER spectrogram they code."""
    _check_host_rows(mc, "decode_melcep", 2)
    check_order(np.shape(mc)[1] - 1, "decode_melcep")
    return _on_device(spectrum_device, mc, fft_size, _alpha(alpha, fs, "decode_melcep"))


def melcep_distortion(mc_a, mc_b):
    """(N, m + 1) rows against (N, m + 1) rows -> (N,) mel-cepstral distortion in dB."""
    _check_host_rows(mc_a, "melcep_distortion", 2)
    if np.shape(mc_a) != np.shape(mc_b):
        raise ValueError("melcep_distortion: rows of shape %s against %s" % (np.shape(mc_a), np.shape(mc_b)))
    return _on_device(lambda rt, a: mcd_db_device(a, rt.to_device(np.ascontiguousarray(mc_b, dtype=np.float64))), mc_a)


@_hip.serialised
def filter_waveform_melcep(fs, x, mc_num, mc_den=None, alpha=None, frame_period=5.0, fft_size=None):
    """x filtered by the envelope of mc_num over that of mc_den ((N, m + 1) rows on x's frame grid; mc_den None: by
    mc_num's alone): a NumPy array like x.  ``fft_size`` None: CheapTrick's for ``fs``."""
    from .cheaptrick import default_fft_size

    x = _hip.host_recording(x, "filter_waveform_melcep")
    _check_host_rows(mc_num, "filter_waveform_melcep", 2)
    if mc_den is not None and np.shape(mc_den) != np.shape(mc_num):
        raise ValueError("filter_waveform_melcep: rows of shape %s against %s" % (np.shape(mc_num), np.shape(mc_den)))
    check_order(np.shape(mc_num)[1] - 1, "filter_waveform_melcep")
    alpha = _alpha(alpha, fs, "filter_waveform_melcep")
    fft_size = default_fft_size(fs) if fft_size is None else fft_size
    rt = _hip.Runtime.get()
    with rt.lock, rt.on_stream():
        num = rt.to_device(np.ascontiguousarray(mc_num, dtype=np.float64))
        den = None if mc_den is None else rt.to_device(np.ascontiguousarray(mc_den, dtype=np.float64))
        out = filter_device(rt, rt.to_device(x), [0, len(x)], fs, frame_period, fft_size, num, den, alpha).cpu().numpy()
    rt.check_flags("filter_waveform_melcep")
    return out
