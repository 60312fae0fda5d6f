"""Line spectral frequencies (LSF): the all-pole code of a spectral envelope.  A row is [log E, w_1 .. w_p] — the log of the
prediction-error gain and p angles in radians, ascending in (0, pi) — and every sorted row is a stable all-pole envelope:
the average of two rows, the MMSE mean of a mixture or an MLPG track is an envelope again, and nothing in a row depends
on the sampling rate, so the code exists where the reference's mel-cepstrum (16 kHz only) does not.

    rows = lsf_device(rt, enc.spectrogram, 40)           # [F][41], resident
    spec = ilsf_device(rt, rows, enc.fft_size)           # [F][K], the all-pole envelope E / |A|^2
    ce = enc.compact(lsf_order=40)                       # CompactEncoding with LSF rows, at any rate

The chain is four kernels: the autocorrelation lags 0..p of a power-spectrum row are a product with a cosine table on the
FP64 matrix cores (wh_feature_matmul), then wh_lpc_levinson, wh_lsf_from_lpc and, on the way back, wh_lsf_envelope
(csrc/wh_lsf.hip).  The arithmetic of the three is a contract (include/world_hip.h) that
tests/_lsf_reference.py states in NumPy and the device reproduces bit for bit; they work on x = cos w, and the only
trigonometry is the three host tables below plus torch.acos / torch.cos / log / exp on the small [F][p] result here.

Rows that a model produced (interpolated, converted, generated) may be out of order or too close: ``min_gap`` (radians)
repairs them before the envelope, in radians: clamp into [gap, pi - gap], a forward pass w[i] = max(w[i], w[i-1] + gap),
the last angle back under pi - gap, and a backward pass w[i] = min(w[i], w[i+1] - gap).  repair_rows states it with
torch's elementwise max / min / + / - (about 2 p + 2 launches, each over one strided column); repair_device is the same
arithmetic in one kernel, wh_lsf_repair (csrc/wh_lsf_chain.hip), one read and one write of the tensor, the same bits.

The voice-conversion chain runs over these rows at every rate: CompactEncoding.dynamic_features /
with_trajectories / align, world.align.align_compact and world.gmm's fit_compact / convert_compact take the kind 'lsf',
and a conversion is scored by the log-spectral distortion of two rows' envelopes on aligned frames — distortion_device,
Alignment.lsd_db — which wh_lsf_distortion forms from the two rows in product form, without either envelope in memory.

The tables and the argument checks are host code and need neither the library nor a GPU."""
import functools

import numpy as np

from . import _hip
from .features import _Tagged, feature_matmul_device

MAX_ORDER = 64
GRID_MAX = 4096


# ---- host ------------------------------------------------------------------------------------------------------------
def check_order(order, where="lsf", k_bins=None):
    """ValueError for an order the kernels do not take: even, 2 .. 64, and (given the bins) at most k_bins - 1 lags."""
    if isinstance(order, bool) or int(order) != order or order < 2 or order > MAX_ORDER or int(order) % 2:
        raise ValueError("%s: the order must be an even integer in [2, %d], got %r" % (where, MAX_ORDER, order))
    if k_bins is not None and (k_bins < 3 or int(order) + 1 > k_bins):
        raise ValueError("%s: %d bins are too few for order %d (lags 0 .. %d of a %d-point spectrum)"
                         % (where, k_bins, order, order, 2 * (k_bins - 1)))
    return int(order)


def check_fft_size(fft_size, where="ilsf"):
    if int(fft_size) != fft_size or fft_size < 4 or int(fft_size) % 2 or fft_size // 2 + 1 > 16385:
        raise ValueError("%s: fft_size must be an even integer in [4, 32768], got %r" % (where, fft_size))
    return int(fft_size) // 2 + 1


@functools.lru_cache(maxsize=16)
def autocorr_table(k_bins, order):
    """[K][p + 1]: power-spectrum row -> lags 0 .. p of irfft(row): w_k cos(2 pi k m / N) / N with N = 2 (K - 1), w = 1 at
    k = 0 and K - 1 and 2 elsewhere (k m is reduced modulo N first, in integers)."""
    n = 2 * (k_bins - 1)
    k = np.arange(k_bins, dtype=np.int64)[:, None]
    m = np.arange(order + 1, dtype=np.int64)[None, :]
    w = np.full((k_bins, 1), 2.0)
    w[0] = w[-1] = 1.0
    return _Tagged(w * np.cos(2 * np.pi * ((k * m) % n) / n) / n)


@functools.lru_cache(maxsize=1)
def grid_table():
    """cos(pi g / 4096), g = 0 .. 4096: the abscissae of the finest root grid; level G is every (4096 / G)-th entry."""
    g = np.cos(np.pi * np.arange(GRID_MAX + 1) / GRID_MAX)
    g[0], g[-1] = 1.0, -1.0
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=16)
def bin_table(k_bins):
    """cos(pi k / (K - 1)): the bins of the envelope in the cosine domain."""
    c = np.cos(np.pi * np.arange(k_bins) / (k_bins - 1))
    c[0], c[-1] = 1.0, -1.0
    c.setflags(write=False)
    return c


# ---- device ----------------------------------------------------------------------------------------------------------
def autocorr_device(rt, spec_d, order):
    """Lags 0 .. order of every row of a power spectrogram [F][K]: [F][order + 1]."""
    _hip.check_rows(rt, "spec", spec_d, "autocorr", 3)
    f, k_bins = (int(v) for v in spec_d.shape)
    check_order(order, "autocorr", k_bins)
    return feature_matmul_device(rt, spec_d, f, k_bins, _hip.ld(spec_d), autocorr_table(k_bins, int(order)))


def levinson_device(rt, r_d, order, want_reflection=False):
    """wh_lpc_levinson on autocorrelation rows [F][>= order + 1]: (a [F][order + 1], E [F], reflection [F][order] or None)."""
    _hip.check_rows(rt, "r", r_d, "levinson", int(order) + 1)
    if int(order) != order or not 1 <= order <= MAX_ORDER:
        raise ValueError("levinson: the order must be an integer in [1, %d], got %r" % (MAX_ORDER, order))
    f, p = int(r_d.shape[0]), int(order)
    a, e = rt.empty((f, p + 1)), rt.empty((f,))
    k = rt.empty((f, p)) if want_reflection else None
    _hip.check(rt.lib.wh_lpc_levinson(rt.ctx, rt.stream(), rt.ptr(r_d), f, _hip.ld(r_d), p, rt.ptr(a), p + 1, rt.ptr(e),
                                      rt.ptr(k), p))
    return a, e, k


def lsf_from_lpc_device(rt, a_d, want_level=False):
    """wh_lsf_from_lpc on predictor rows [F][p + 1]: the cosines of the line spectral frequencies [F][p], descending;
    ``want_level``: (x, level int32 [F]) — the grid level that found every root of the frame, 0 for a flagged one."""
    _hip.check_rows(rt, "a", a_d, "lsf_from_lpc", 3)
    f, p = int(a_d.shape[0]), check_order(int(a_d.shape[1]) - 1, "lsf_from_lpc")
    x = rt.empty((f, p))
    level = rt.empty((f,), dtype=rt.torch.int32) if want_level else None
    grid = grid_table()
    _hip.check(rt.lib.wh_lsf_from_lpc(rt.ctx, rt.stream(), rt.ptr(a_d), f, _hip.ld(a_d), p, _hip.f64p(grid), len(grid),
                                      rt.ptr(x), p, rt.ptr(level)))
    return (x, level) if want_level else x


def envelope_device(rt, ex_d, k_bins):
    """wh_lsf_envelope on rows [E, x_1 .. x_p] (gain and COSINES): the power spectrum [F][k_bins]."""
    _hip.check_rows(rt, "rows", ex_d, "lsf_envelope", 3)
    f, p = int(ex_d.shape[0]), check_order(int(ex_d.shape[1]) - 1, "lsf_envelope")
    out = rt.empty((f, int(k_bins)))
    _hip.check(rt.lib.wh_lsf_envelope(rt.ctx, rt.stream(), rt.ptr(ex_d), f, _hip.ld(ex_d), p, _hip.f64p(bin_table(int(k_bins))),
                                      int(k_bins), rt.ptr(out), int(k_bins)))
    return out


def lpc_device(rt, spec_d, order):
    """Power spectrogram [F][K] -> (a [F][order + 1] with a[0] = 1, E [F], reflection coefficients [F][order])."""
    with rt.lock, rt.on_stream():
        return levinson_device(rt, autocorr_device(rt, spec_d, order), order, want_reflection=True)


def lsf_device(rt, spec_d, order):
    """Power spectrogram [F][K] (BatchEncoding.spectrogram is one) -> rows [F][order + 1] = [log E, w_1 .. w_p], radians
    ascending.  A row that is not positive and finite gives a NaN row and the deferred flag FLAG_LSF; an all-zero row
    gives log E = -inf and the LSFs of A = 1."""
    torch = rt.torch
    with rt.lock, rt.on_stream():
        a, e, _ = levinson_device(rt, autocorr_device(rt, spec_d, order), order)
        x = lsf_from_lpc_device(rt, a)
        return torch.cat([torch.log(e)[:, None], torch.acos(x)], dim=1)


def repair_rows(torch, w, min_gap):
    """The angles [F][p] made decodable: inside [gap, pi - gap] and at least gap apart (module docstring)."""
    if not min_gap > 0:
        return w
    w = torch.clamp(w, min=float(min_gap), max=float(np.pi - min_gap)).contiguous()
    p = int(w.shape[1])
    for i in range(1, p):
        w[:, i] = torch.maximum(w[:, i], w[:, i - 1] + float(min_gap))
    w[:, p - 1] = torch.clamp(w[:, p - 1], max=float(np.pi - min_gap))
    for i in range(p - 2, -1, -1):
        w[:, i] = torch.minimum(w[:, i], w[:, i + 1] - float(min_gap))
    return w


def check_min_gap(min_gap, p, where="repair"):
    """ValueError unless 0 <= min_gap < pi / (p + 2): p angles at least that far apart and from 0 and pi must fit."""
    if not 0 <= float(min_gap) < np.pi / (int(p) + 2):
        raise ValueError("%s: min_gap must be in [0, pi / (p + 2)), got %r" % (where, min_gap))
    return float(min_gap)


def repair_device(rt, w, min_gap, want_changed=False, out=None):
    """wh_lsf_repair: the angles [F][p] (a column slice of the rows is fine) made decodable, in one pass — repair_rows'
    arithmetic step for step, the same bits.  ``min_gap`` > 0.  ``out``: where to (w itself: in place); a new tensor when
    None.  ``want_changed``: (angles, changed int32 [F]) — how many angles of each frame the repair moved."""
    _hip.check_rows(rt, "w", w, "repair", 2)
    f, p = int(w.shape[0]), int(w.shape[1])
    if p > MAX_ORDER:
        raise ValueError("repair: rows of %d angles; the kernel takes 2 .. %d" % (p, MAX_ORDER))
    gap = check_min_gap(min_gap, p)
    if not gap > 0:
        raise ValueError("repair: min_gap must be positive, got %r" % (min_gap,))
    with rt.lock, rt.on_stream():
        if out is None:
            out = rt.empty((f, p))
        else:
            _hip.check_rows(rt, "out", out, "repair", 2)
            if tuple(out.shape) != (f, p):
                raise ValueError("repair: out must be %s, got %s" % ((f, p), tuple(out.shape)))
        changed = rt.empty((f,), dtype=rt.torch.int32) if want_changed else None
        _hip.check(rt.lib.wh_lsf_repair(rt.ctx, rt.stream(), rt.ptr(w), f, _hip.ld(w), p, gap, float(np.pi - gap), rt.ptr(out),
                                        _hip.ld(out), rt.ptr(changed)))
    return (out, changed) if want_changed else out


def ilsf_device(rt, rows_d, fft_size, min_gap=0.0):
    """Rows [F][p + 1] = [log E, w_1 .. w_p] -> the power spectrum [F][fft_size // 2 + 1].  ``min_gap`` = 0: the rows are
    used as they are; > 0: repaired first (module docstring; wh_lsf_repair)."""
    k_bins = check_fft_size(fft_size)
    _hip.check_rows(rt, "rows", rows_d, "ilsf", 3)
    p = check_order(int(rows_d.shape[1]) - 1, "ilsf")
    gap = check_min_gap(min_gap, p, "ilsf")
    torch = rt.torch
    with rt.lock, rt.on_stream():
        w = repair_device(rt, rows_d[:, 1:], gap) if gap > 0 else rows_d[:, 1:]
        ex = torch.cat([torch.exp(rows_d[:, :1]), torch.cos(w)], dim=1)
        return envelope_device(rt, ex, k_bins)


LSD_SCALE = 10.0 / np.log(10.0)


def _index(rt, idx, n_pairs, name):
    if idx is None:
        return None
    if idx.dim() != 1 or idx.dtype != rt.torch.int64 or not idx.is_contiguous() or int(idx.shape[0]) != n_pairs:
        raise ValueError("lsf_distortion: %s must be a contiguous int64 tensor [%d], got %s %s"
                         % (name, n_pairs, idx.dtype, tuple(idx.shape)))
    return idx


def distortion_sums_device(rt, ex_a, ex_b, k_bins, idx_a=None, idx_b=None):
    """wh_lsf_distortion on rows [., x_1 .. x_p] (COSINES, as envelope_device takes them): [n_pairs][2] = (sum over the
    bins of t, sum of t * t), t = log(A2_a / A2_b).  Pair n is row idx_a[n] against row idx_b[n] (int64 device tensors,
    batch-global frame indices as Alignment.path_a / path_b hold them), or row n where an index is None."""
    _hip.check_rows(rt, "rows_a", ex_a, "lsf_distortion", 3)
    _hip.check_rows(rt, "rows_b", ex_b, "lsf_distortion", 3)
    p = check_order(int(ex_a.shape[1]) - 1, "lsf_distortion")
    if int(ex_b.shape[1]) != p + 1:
        raise ValueError("lsf_distortion: rows of order %d against rows of order %d" % (p, int(ex_b.shape[1]) - 1))
    if idx_a is None and idx_b is None and int(ex_a.shape[0]) != int(ex_b.shape[0]):
        raise ValueError("lsf_distortion: %d rows against %d and no indices" % (int(ex_a.shape[0]), int(ex_b.shape[0])))
    n_pairs = int((idx_a if idx_a is not None else idx_b if idx_b is not None else ex_a).shape[0])
    idx_a, idx_b = _index(rt, idx_a, n_pairs, "idx_a"), _index(rt, idx_b, n_pairs, "idx_b")
    with rt.lock, rt.on_stream():
        out = rt.empty((n_pairs, 2))
        _hip.check(rt.lib.wh_lsf_distortion(rt.ctx, rt.stream(), rt.ptr(ex_a), int(ex_a.shape[0]), _hip.ld(ex_a), rt.ptr(ex_b),
                                            int(ex_b.shape[0]), _hip.ld(ex_b), p, rt.ptr(idx_a), rt.ptr(idx_b), n_pairs,
                                            _hip.f64p(bin_table(int(k_bins))), int(k_bins), rt.ptr(out)))
    return out


def distortion_db(torch, g, s1, s2, k_bins, gain=True):
    """The log-spectral distortion in dB from the gain difference g = log E_a - log E_b and the kernel's two sums (torch
    or NumPy: ``torch`` is the module the arrays belong to).  The envelope is S = E / A2, so
    ln S_a - ln S_b = g - ln(A2_a / A2_b) = g - t: the gain enters with the OPPOSITE sign of t.  Per pair,
        gain=True:   c sqrt(max(0, mean_k (g - t)^2))      = c sqrt(max(0, g^2 - 2 g s1 / K + s2 / K))
        gain=False:  c sqrt(max(0, var_k t))               = c sqrt(max(0, s2 / K - (s1 / K)^2))
    with c = 10 / ln 10: the RMS over the bins of the dB difference, and the same with the best constant gain taken out
    (the distortion of the spectral SHAPE)."""
    m1, m2 = s1 / k_bins, s2 / k_bins
    v = (g * g - 2.0 * g * m1 + m2) if gain else (m2 - m1 * m1)
    return LSD_SCALE * torch.sqrt(torch.maximum(v, torch.zeros_like(v)))


def distortion_device(rt, rows_a, rows_b, fft_size, idx_a=None, idx_b=None, gain=True):
    """The log-spectral distortion in dB of pairs of rows [log E, w_1 .. w_p] (radians): [n_pairs], the RMS over the
    fft_size // 2 + 1 bins of 10 log10(S_a / S_b) of the two all-pole envelopes, neither of which is written
    (wh_lsf_distortion).  Pair n is row idx_a[n] of rows_a against row idx_b[n] of rows_b, or row n where an index is
    None.  ``gain=False`` leaves the best constant gain out.  The sign of the cross term: distortion_db."""
    k_bins = check_fft_size(fft_size, "lsf_distortion")
    _hip.check_rows(rt, "rows_a", rows_a, "lsf_distortion", 3)
    _hip.check_rows(rt, "rows_b", rows_b, "lsf_distortion", 3)
    torch = rt.torch
    with rt.lock, rt.on_stream():
        # the kernel takes rows of p + 1 columns and does not read column 0: the cosines go into columns 1 .. p of a
        # tensor whose column 0 is left as it is allocated
        ex_a, ex_b = rt.empty(tuple(rows_a.shape)), rt.empty(tuple(rows_b.shape))
        torch.cos(rows_a[:, 1:], out=ex_a[:, 1:])
        torch.cos(rows_b[:, 1:], out=ex_b[:, 1:])
        s = distortion_sums_device(rt, ex_a, ex_b, k_bins, idx_a, idx_b)
        ga = rows_a[:, 0] if idx_a is None else _gather(torch, rows_a[:, 0], idx_a)
        gb = rows_b[:, 0] if idx_b is None else _gather(torch, rows_b[:, 0], idx_b)
        return distortion_db(torch, ga - gb, s[:, 0], s[:, 1], k_bins, gain)


def _gather(torch, col, idx):
    """col[idx] with NaN where an index is outside the column (the kernel's answer for such a pair)."""
    n = int(col.shape[0])
    ok = (idx >= 0) & (idx < n)
    if n == 0:
        return torch.full(idx.shape, float("nan"), dtype=col.dtype, device=col.device)
    v = col.index_select(0, torch.where(ok, idx, torch.zeros_like(idx)))
    return torch.where(ok, v, torch.full_like(v, float("nan")))


# ---- NumPy forms (World.encode_lsf / decode_lsf / encode_lpc) ---------------------------------------------------------
@_hip.serialised
def _on_device(fn, x, *a, **kw):
    rt = _hip.Runtime.get()
    out = fn(rt, rt.to_device(np.ascontiguousarray(x, dtype=np.float64)), *a, **kw)
    rt.check_flags(fn.__name__)
    return tuple(t.cpu().numpy() for t in out) if isinstance(out, tuple) else out.cpu().numpy()


def _check_host_rows(x, where, min_cols):
    if np.ndim(x) != 2 or np.shape(x)[1] < min_cols:
        raise ValueError("%s: expected (N frames, >= %d columns), got shape %s" % (where, min_cols, np.shape(x)))


def encode_lsf(spec, order=24):
    """(N, D) power spectrogram -> (N, order + 1) rows [log E, w_1 .. w_p]."""
    _check_host_rows(spec, "encode_lsf", 3)
    check_order(order, "encode_lsf", np.shape(spec)[1])
    return _on_device(lsf_device, spec, int(order))


def decode_lsf(lsf, fft_size, min_gap=0.0):
    """(N, p + 1) rows -> (N, fft_size / 2 + 1) power spectrogram."""
    check_fft_size(fft_size, "decode_lsf")
    _check_host_rows(lsf, "decode_lsf", 3)
    check_order(np.shape(lsf)[1] - 1, "decode_lsf")
    return _on_device(ilsf_device, lsf, int(fft_size), min_gap)


def lsf_distortion(lsf_a, lsf_b, fft_size, gain=True):
    """(N, p + 1) rows against (N, p + 1) rows -> (N,) log-spectral distortion in dB, frame by frame."""
    check_fft_size(fft_size, "lsf_distortion")
    _check_host_rows(lsf_a, "lsf_distortion", 3)
    _check_host_rows(lsf_b, "lsf_distortion", 3)
    if np.shape(lsf_a) != np.shape(lsf_b):
        raise ValueError("lsf_distortion: rows of shape %s against %s" % (np.shape(lsf_a), np.shape(lsf_b)))
    check_order(np.shape(lsf_a)[1] - 1, "lsf_distortion")
    return _on_device(lambda rt, a: distortion_device(rt, a, rt.to_device(np.ascontiguousarray(lsf_b, dtype=np.float64)),
                                                      int(fft_size), gain=gain), lsf_a)


def encode_lpc(spec, order=24):
    """(N, D) power spectrogram -> (a (N, order + 1), E (N,), reflection coefficients (N, order))."""
    _check_host_rows(spec, "encode_lpc", 3)
    check_order(order, "encode_lpc", np.shape(spec)[1])
    return _on_device(lpc_device, spec, int(order))
