"""Dynamic features and maximum-likelihood parameter generation (MLPG): the two halves between WORLD parameter tracks and
a statistical model of them.  Such a model — an acoustic model for synthesis, a conversion model between two aligned
speakers — is trained on static + delta + delta-delta rows of a CompactEncoding's columns (mel-cepstrum, band
aperiodicity, log-f0) and predicts a mean and a variance for each; MLPG turns those back into the one track that is most
likely under them: per utterance and column the banded symmetric positive definite system

    (sum_w W_w' P_w W_w) c = sum_w W_w' P_w mu_w

The kernels are behind wh_delta_features / wh_mlpg (csrc/wh_mlpg.hip); the arithmetic is a contract (include/world_hip.h,
DESIGN section 15) that tests/_mlpg_reference.py states in NumPy and the device reproduces bit for bit.  A system's result
does not depend on the batch it is in.

``batch`` is any descriptor from rt.make_batch: its "utterances" are the stretches no window may reach across.  A caller
who generates log-f0 over the voiced runs only passes the runs as utterances (frame offsets of the runs over the
gathered voiced rows); nothing more is built for that here.

The argument checks and the workspace grouping are host code and need neither the library nor a GPU."""
import numpy as np

from . import _hip

# the windows every HTS-style toolkit ships: static, delta, delta-delta
HTS_WINDOWS = ((0.0, 1.0, 0.0), (-0.5, 0.0, 0.5), (1.0, -2.0, 1.0))
MAX_WINDOWS = 4
MAX_HALF = 2
DEFAULT_MAX_WORKSPACE_BYTES = 4 << 30


# ---- host ------------------------------------------------------------------------------------------------------------
def check_windows(windows, where="dynamics"):
    """(win [n_win][2L + 1] float64 C-contiguous, L) or ValueError: 1 .. 4 windows of one half-width L in {0, 1, 2}, window 0
    the static one (centre tap exactly 1.0, every other tap exactly 0.0 — it gives the system full rank)."""
    try:
        rows = [np.asarray(w, dtype=np.float64) for w in windows]
    except (TypeError, ValueError):
        raise ValueError("%s: windows must be a sequence of tap sequences" % where)
    if not 1 <= len(rows) <= MAX_WINDOWS:
        raise ValueError("%s: 1 .. %d windows, got %d" % (where, MAX_WINDOWS, len(rows)))
    if any(r.ndim != 1 for r in rows) or len({len(r) for r in rows}) != 1:
        raise ValueError("%s: the windows must all have the same half-width (pad the shorter ones with zeros), got lengths %s"
                         % (where, [int(np.size(r)) for r in rows]))
    n = len(rows[0])
    if n % 2 != 1 or n // 2 > MAX_HALF:
        raise ValueError("%s: windows of 1, 3 or 5 taps (half-width 0 .. %d), got %d taps" % (where, MAX_HALF, n))
    win = np.ascontiguousarray(np.stack(rows))
    if not np.all(np.isfinite(win)):
        raise ValueError("%s: window taps must be finite" % where)
    static = np.zeros(n)
    static[n // 2] = 1.0
    if not np.array_equal(win[0], static):
        raise ValueError("%s: window 0 must be the static window (centre tap 1.0, every other tap 0.0), got %s"
                         % (where, win[0].tolist()))
    return win, n // 2


def workspace_bytes(frames, d, half):
    """What wh_mlpg takes of the context's scratch for ``frames`` frames of ``d`` columns: the multipliers of the
    factorisation, B = 2 * half doubles per frame and column (128 MB for 2001 x 100 frames x 40 columns at half = 1)."""
    return 8 * int(frames) * int(d) * 2 * int(half)


def plan_groups(n_frames, d, half, max_workspace_bytes=DEFAULT_MAX_WORKSPACE_BYTES):
    """Consecutive utterances [u0, u1) per wh_mlpg call: as many as fit ``max_workspace_bytes`` of multipliers, taken in
    order; an utterance that is larger than the limit on its own is a group of one."""
    groups, u0, used = [], 0, 0
    for u, n in enumerate(n_frames):
        need = workspace_bytes(n, d, half)
        if u > u0 and used + need > max_workspace_bytes:
            groups.append((u0, u))
            u0, used = u, 0
        used += need
    if len(n_frames) > u0:
        groups.append((u0, len(n_frames)))
    return groups


def check_rows(name, shape, frames, width, where):
    if len(shape) != 2 or int(shape[0]) != frames or int(shape[1]) != width:
        raise ValueError("%s: %s must be [%d frames][%d], got %s" % (where, name, frames, width, tuple(shape)))


def check_mlpg_shapes(mean_shape, var_shape, frames, n_win, where="mlpg"):
    """ValueError for shapes wh_mlpg cannot take.  Returns (d, per_frame): the columns of a track, and whether ``var``
    holds a row per frame ([F][n_win d]) or one row for all ([n_win d])."""
    if len(mean_shape) != 2 or int(mean_shape[0]) != frames:
        raise ValueError("%s: mean must be [%d frames][n_win * d], got %s" % (where, frames, tuple(mean_shape)))
    width = int(mean_shape[1])
    if width < n_win or width % n_win:
        raise ValueError("%s: rows of %d columns do not hold %d windows of the same d columns" % (where, width, n_win))
    if tuple(int(v) for v in var_shape) == (width,):
        return width // n_win, False
    if tuple(int(v) for v in var_shape) == (frames, width):
        return width // n_win, True
    raise ValueError("%s: var must be [%d][%d] like mean, or [%d] (one row of variances for every frame), got %s"
                     % (where, frames, width, width, tuple(var_shape)))


# ---- device ----------------------------------------------------------------------------------------------------------
def _check_tensor(rt, name, t, where):
    if t.dtype != rt.torch.float64 or t.stride(-1) != 1:
        raise ValueError("%s: %s must be a float64 tensor with unit column stride, got %s strides %s"
                         % (where, name, t.dtype, tuple(t.stride())))


def delta_features_device(rt, batch, x, windows=HTS_WINDOWS):
    """x: float64 device tensor [frames][d] with unit column stride (a column slice of a wider tensor is fine) ->
    [frames][n_win * d], column w * d + c the window w over column c; a window never reaches across an utterance of
    ``batch`` (the tap is dropped, as np.correlate(..., 'same') does)."""
    win, half = check_windows(windows, "delta_features")
    if x.dim() != 2 or int(x.shape[0]) != batch.total_frames or int(x.shape[1]) < 1:
        raise ValueError("delta_features: x must be [%d frames][d >= 1], got %s" % (batch.total_frames, tuple(x.shape)))
    _check_tensor(rt, "x", x, "delta_features")
    d = int(x.shape[1])
    with rt.lock, rt.on_stream():
        out = rt.empty((batch.total_frames, len(win) * d))
        _hip.check(rt.lib.wh_delta_features(rt.ctx, rt.stream(), batch.handle, rt.ptr(x), int(x.stride(0)) if x.shape[0] > 1 else d,
                                            d, len(win), half, _hip.f64p(win), rt.ptr(out), len(win) * d))
    return out


def _sub_batch(rt, batch, u0, u1):
    fo = batch.frame_off[u0:u1 + 1] - batch.frame_off[u0]
    return rt.make_batch(np.zeros(u1 - u0 + 1, dtype=np.int64), fo)


def mlpg_device(rt, batch, mean, var, windows=HTS_WINDOWS, max_workspace_bytes=DEFAULT_MAX_WORKSPACE_BYTES,
                want_pivots=False):
    """The maximum-likelihood track of every utterance of ``batch`` and every column: mean [frames][n_win * d] (float64
    device tensor, unit column stride; column w * d + c is window w of column c, as delta_features_device lays them
    out), var the same shape or [n_win * d] (one row of variances for every frame: the global-variance case) -> [frames][d].
    Variances must be positive and finite; where they are not, that system's track is unspecified and the deferred flag
    FLAG_MLPG_PIVOT is raised (rt.take_flags / check_flags), the other systems are unaffected.  The multipliers take
    workspace_bytes(frames, d, L) of the context's scratch, and the utterances are handed to the kernel in consecutive
    groups (plan_groups) that keep that under ``max_workspace_bytes``; a result does not depend on its group.
    ``want_pivots``: returns (track, pivots [frames][d]) — the d[t] of the factorisation, a test hook."""
    win, half = check_windows(windows, "mlpg")
    n_win = len(win)
    d, per_frame = check_mlpg_shapes(tuple(mean.shape), tuple(var.shape), batch.total_frames, n_win)
    _check_tensor(rt, "mean", mean, "mlpg")
    _check_tensor(rt, "var", var, "mlpg")
    n_utt = batch.n_utt
    fo = batch.frame_off
    groups = plan_groups(np.diff(fo), d, half, max_workspace_bytes)
    ldm = int(mean.stride(0)) if mean.shape[0] > 1 else n_win * d
    ldv = (int(var.stride(0)) if var.shape[0] > 1 else n_win * d) if per_frame else 0
    with rt.lock, rt.on_stream():
        out = rt.empty((batch.total_frames, d))
        piv = rt.empty((batch.total_frames, d)) if want_pivots else None
        for u0, u1 in groups:
            f0, f1 = int(fo[u0]), int(fo[u1])
            if f1 == f0:
                continue
            g = batch if (u0, u1) == (0, n_utt) else _sub_batch(rt, batch, u0, u1)
            _hip.check(rt.lib.wh_mlpg(rt.ctx, rt.stream(), g.handle, rt.ptr(mean[f0:f1]), ldm,
                                      rt.ptr(var[f0:f1] if per_frame else var), ldv, d, n_win, half, _hip.f64p(win),
                                      rt.ptr(out[f0:f1]), d, rt.ptr(piv[f0:f1]) if want_pivots else None))
    return (out, piv) if want_pivots else out


# ---- CompactEncoding (world/compact.py binds these two as methods) -------------------------------------------------------
def compact_dynamic_features(ce, windows=HTS_WINDOWS):
    """CompactEncoding.dynamic_features: see there."""
    check_windows(windows, "dynamic_features")
    if ce.rt is None:
        raise ValueError("dynamic_features: the encoding is on the host; to_device(rt) first")
    if ce.mcep is None and ce.lsf is None:
        raise ValueError("dynamic_features: the encoding keeps the dense spectrogram (compact(n0=None)): no mel-cepstrum")
    rt = ce.rt
    key = "mcep" if ce.lsf is None else "lsf"  # (LSF rows: the p + 1 columns [log E, w_1 .. w_p])
    with rt.lock, rt.on_stream():
        batch = rt.make_batch(np.zeros(ce.n_utt + 1, dtype=np.int64), ce.frame_off)
        return {key: delta_features_device(rt, batch, getattr(ce, key), windows),
                "band_ap": delta_features_device(rt, batch, ce.band_ap, windows)}


def compact_with_trajectories(ce, mcep=None, band_ap=None, windows=HTS_WINDOWS, lsf=None, min_gap=None):
    """CompactEncoding.with_trajectories: see there."""
    win, _ = check_windows(windows, "with_trajectories")
    if mcep is not None and ce.lsf is not None:
        raise ValueError("with_trajectories: mcep= on an encoding that holds line spectral frequencies: pass lsf=")
    if lsf is not None and ce.lsf is None:
        raise ValueError("with_trajectories: lsf= on an encoding that holds no line spectral frequencies (kind %r)" % ce.kind)
    if ce.rt is None:
        raise ValueError("with_trajectories: the encoding is on the host; to_device(rt) first")
    if mcep is not None and ce.mcep is None:
        raise ValueError("with_trajectories: the encoding keeps the dense spectrogram (compact(n0=None)): no mel-cepstrum")
    if lsf is not None:
        from .lsf import check_min_gap, repair_device
        if min_gap is None or not check_min_gap(min_gap, ce.lsf_order, "with_trajectories") > 0:
            raise ValueError("with_trajectories: lsf= needs min_gap > 0 (radians): a generated track decodes only after "
                             "the repair")
    rt = ce.rt
    nf = ce.total_frames
    for name, pair, width in (("mcep", mcep, None if ce.mcep is None else int(ce.mcep.shape[1])),
                              ("lsf", lsf, None if ce.lsf is None else int(ce.lsf.shape[1])),
                              ("band_ap", band_ap, int(ce.band_ap.shape[1]))):
        if pair is None:
            continue
        if not isinstance(pair, (tuple, list)) or len(pair) != 2:
            raise ValueError("with_trajectories: %s must be (mean, var) or None" % name)
        check_rows(name + " mean", tuple(pair[0].shape), nf, len(win) * width, "with_trajectories")
        check_mlpg_shapes(tuple(pair[0].shape), tuple(pair[1].shape), nf, len(win), "with_trajectories: " + name)
    with rt.lock, rt.on_stream():
        batch = rt.make_batch(np.zeros(ce.n_utt + 1, dtype=np.int64), ce.frame_off)
        arrays = dict(ce._tensors())
        if mcep is not None:
            arrays["mcep"] = mlpg_device(rt, batch, mcep[0], mcep[1], windows)
        if lsf is not None:  # the gain and the angles are generated alike; the angles are then made decodable, in place
            rows = mlpg_device(rt, batch, lsf[0], lsf[1], windows)
            repair_device(rt, rows[:, 1:], min_gap, out=rows[:, 1:])
            arrays["lsf"] = rows
        if band_ap is not None:
            arrays["band_ap"] = mlpg_device(rt, batch, band_ap[0], band_ap[1], windows)
    return ce._like(rt, arrays, None if ce.tp_host is None else np.array(ce.tp_host))


# ---- NumPy forms (World.delta_features / World.mlpg) ------------------------------------------------------------------------
def _as_list(x, where):
    """([arrays [T][.]], single): one utterance or a list of them."""
    single = isinstance(x, np.ndarray) and x.ndim == 2
    parts = [np.asarray(p, dtype=np.float64) for p in ([x] if single else list(x))]
    for n, p in enumerate(parts):
        if p.ndim != 2:
            raise ValueError("%s: utterance %d must be [T][columns], got shape %s" % (where, n, p.shape))
    if len({p.shape[1] for p in parts}) > 1:
        raise ValueError("%s: the utterances' rows differ in width: %s" % (where, sorted({p.shape[1] for p in parts})))
    return parts, single


def delta_features_numpy(x, windows=HTS_WINDOWS):
    check_windows(windows, "delta_features")
    parts, single = _as_list(x, "delta_features")
    if not parts:
        return []
    if parts[0].shape[1] < 1:
        raise ValueError("delta_features: rows without columns")
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    if off[-1] == 0:
        out = [np.zeros((0, len(windows) * parts[0].shape[1])) for _ in parts]
        return out[0] if single else out
    rt = _hip.Runtime.get()
    with rt.lock, rt.on_stream():
        batch = rt.make_batch(np.zeros(len(parts) + 1, dtype=np.int64), off)
        y = rt.to_host(delta_features_device(rt, batch, rt.to_device(np.concatenate(parts)), windows))
    out = [np.array(y[off[u]:off[u + 1]]) for u in range(len(parts))]
    return out[0] if single else out


def mlpg_numpy(mean, var, windows=HTS_WINDOWS):
    win, _ = check_windows(windows, "mlpg")
    means, single = _as_list(mean, "mlpg")
    if not means:
        return []
    width = means[0].shape[1]
    one_row = isinstance(var, np.ndarray) and var.ndim == 1
    if one_row:
        check_mlpg_shapes((len(means[0]), width), var.shape, len(means[0]), len(win))
        var_all = np.ascontiguousarray(var, dtype=np.float64)
    else:
        vs, v_single = _as_list(var, "mlpg")
        if v_single != single or len(vs) != len(means):
            raise ValueError("mlpg: var must be given like mean (one utterance or a list of as many), or as one row [n_win * d]")
        for m, v in zip(means, vs):
            check_mlpg_shapes(m.shape, v.shape, len(m), len(win))
        var_all = np.concatenate(vs)
    d = check_mlpg_shapes((len(means[0]), width), (width,), len(means[0]), len(win))[0]
    off = np.concatenate([[0], np.cumsum([len(p) for p in means])]).astype(np.int64)
    if off[-1] == 0:
        out = [np.zeros((0, d)) for _ in means]
        return out[0] if single else out
    rt = _hip.Runtime.get()
    with rt.lock, rt.on_stream():
        batch = rt.make_batch(np.zeros(len(means) + 1, dtype=np.int64), off)
        c = rt.to_host(mlpg_device(rt, batch, rt.to_device(np.concatenate(means)), rt.to_device(var_all), windows))
    rt.check_flags("mlpg")
    out = [np.array(c[off[u]:off[u + 1]]) for u in range(len(means))]
    return out[0] if single else out
