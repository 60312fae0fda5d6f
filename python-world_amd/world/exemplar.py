"""Exemplar-based voice conversion by frame selection (unit selection at frame level: Dutoit et al. 2007, Sündermann et
al. 2006): the target speaker's aligned frames are kept as a database, every source frame takes the K entries whose source
side is nearest, and a Viterbi pass picks one per frame, trading closeness against the continuity of the chosen target
frames.  Every converted envelope is a frame the target speaker produced: nothing is averaged, which is the remedy for
the joint-density GMM's over-smoothing that needs no iteration and no tolerance.  The kernels are behind wh_knn and
wh_frame_select (csrc/wh_exemplar.hip); the arithmetic is a contract (include/world_hip.h) that
tests/_exemplar_reference.py states in NumPy and the device reproduces bit for bit.

The database, its scales, the argument checks and the .npz form are host code and need neither the library nor a GPU."""
import numpy as np

from . import _hip
from .dynamics import check_windows
from .gmm import CONVERSION_WINDOWS

# the search kernel's tiling (csrc/wh_exemplar.hip: kKnnTileQ, kKnnTileR, kKnnStrip) and the walk back's piece
# (kFsChunk); the tests put their shapes around these, and tests/test_exemplar_host.py holds the two files together
TILE_Q = 64
TILE_R = 64
STRIP = 16
CHUNK = 256
MAX_D = 160
MAX_K = 32
MAX_DY = 64
MAX_SPLITS = 65535
MODES = ("frames", "mlpg")


# ---- host ----------------------------------------------------------------------------------------------------------
def column_scales(rows):
    """1 / std per column over the rows (NumPy, population std); 1.0 for a column whose std is zero or not finite."""
    rows = np.asarray(rows, dtype=np.float64)
    with np.errstate(all="ignore"):
        std = np.std(rows, axis=0) if rows.shape[0] else np.zeros(rows.shape[1])
        ok = np.isfinite(std) & (std > 0.0)
        return np.where(ok, 1.0 / np.where(ok, std, 1.0), 1.0)


def chain_succ(utt_off):
    """succ[r] = r + 1 inside an utterance, r at its last frame (int32)."""
    utt_off = np.asarray(utt_off, dtype=np.int64)
    succ = np.arange(1, int(utt_off[-1]) + 1, dtype=np.int32)
    last = utt_off[1:][np.diff(utt_off) > 0] - 1
    succ[last] = last
    return succ


def check_knn_args(n_q, dq, n_db, ddb, k, splits, where="knn"):
    if dq != ddb:
        raise ValueError("%s: queries of %d columns against a database of %d" % (where, dq, ddb))
    if not 1 <= dq <= MAX_D:
        raise ValueError("%s: rows of %d columns; the kernel takes 1 .. %d" % (where, dq, MAX_D))
    if isinstance(k, bool) or int(k) != k or not 1 <= k <= MAX_K:
        raise ValueError("%s: k must be an integer in [1, %d], got %r" % (where, MAX_K, k))
    if n_db > 2 ** 31 - 1:
        raise ValueError("%s: a database of %d rows; the indices are int32" % (where, n_db))
    if isinstance(splits, bool) or int(splits) != splits or not 0 <= splits <= MAX_SPLITS:
        raise ValueError("%s: splits must be an integer in [0, %d], got %r" % (where, MAX_SPLITS, splits))


def check_select_args(frames, idx_shape, dist_shape, y_shape, n_succ, weight, where="select"):
    if len(idx_shape) != 2 or tuple(idx_shape) != tuple(dist_shape) or int(idx_shape[0]) != frames:
        raise ValueError("%s: idx and dist must both be [%d frames][k], got %s and %s"
                         % (where, frames, tuple(idx_shape), tuple(dist_shape)))
    if not 1 <= int(idx_shape[1]) <= MAX_K:
        raise ValueError("%s: %d candidates per frame; the kernel takes 1 .. %d" % (where, int(idx_shape[1]), MAX_K))
    if len(y_shape) != 2 or not 1 <= int(y_shape[1]) <= MAX_DY:
        raise ValueError("%s: y must be [rows][1 .. %d], got %s" % (where, MAX_DY, tuple(y_shape)))
    if n_succ != int(y_shape[0]):
        raise ValueError("%s: succ has %d entries for %d rows" % (where, n_succ, int(y_shape[0])))
    if isinstance(weight, bool) or not (np.isfinite(weight) and weight >= 0.0):
        raise ValueError("%s: the weight must be finite and >= 0, got %r" % (where, weight))


class FrameDatabase:
    """The target speaker's aligned frames (plain NumPy, like JointGMM): row r is target frame r of the training batch;
    ``y`` [R][n_win d] its static + dynamic rows, ``x`` [R][n_win d] the source's rows at the aligned frame, ``succ`` [R]
    the row that follows r in the target recording (r itself at an utterance's last frame), ``scale_x`` / ``scale_y``
    per-column factors under which distances are taken, ``utt_off`` [U + 1] the rows of the training utterances.  ``kind``
    'mcep' (mel-cepstral coefficients 1 .. n0-1) or 'lsf' (the ``lsf_order`` angles; ``lsf_min_gap`` as JointGMM's)."""

    def __init__(self, x, y, succ, scale_x, scale_y, utt_off, windows=CONVERSION_WINDOWS, kind="mcep", lsf_order=None,
                 lsf_min_gap=None):
        if kind not in ("mcep", "lsf"):
            raise ValueError("FrameDatabase: kind must be 'mcep' or 'lsf', got %r" % (kind,))
        if (kind == "lsf") != (lsf_order is not None) or (kind == "lsf") != (lsf_min_gap is not None):
            raise ValueError("FrameDatabase: lsf_order and lsf_min_gap belong to kind 'lsf' and to no other")
        win, _ = check_windows(windows, "FrameDatabase")
        self.kind = kind
        self.lsf_order = None if lsf_order is None else int(lsf_order)
        self.lsf_min_gap = None if lsf_min_gap is None else float(lsf_min_gap)
        self.windows = tuple(tuple(float(v) for v in w) for w in win)
        self.x = np.ascontiguousarray(x, dtype=np.float64)
        self.y = np.ascontiguousarray(y, dtype=np.float64)
        self.succ = np.ascontiguousarray(succ, dtype=np.int32)
        self.scale_x = np.ascontiguousarray(scale_x, dtype=np.float64)
        self.scale_y = np.ascontiguousarray(scale_y, dtype=np.float64)
        self.utt_off = np.ascontiguousarray(utt_off, dtype=np.int64)
        if self.x.ndim != 2 or self.x.shape != self.y.shape:
            raise ValueError("FrameDatabase: x and y must both be [rows][columns], got %s and %s" % (self.x.shape, self.y.shape))
        r, w = self.x.shape
        n_win = len(win)
        if r < 1 or w < n_win or w % n_win or w > MAX_D or w // n_win > MAX_DY:
            raise ValueError("FrameDatabase: %d row(s) of %d columns for %d windows; the kernels take 1 .. %d columns, %d of "
                             "them static" % (r, w, n_win, MAX_D, MAX_DY))
        if r > 2 ** 31 - 1:
            raise ValueError("FrameDatabase: %d rows; the indices are int32" % r)
        if self.succ.shape != (r,) or self.scale_x.shape != (w,) or self.scale_y.shape != (w,):
            raise ValueError("FrameDatabase: succ must be [%d], the scales [%d]" % (r, w))
        if np.any(self.succ < 0) or np.any(self.succ >= r):
            raise ValueError("FrameDatabase: succ points outside the database")
        if (self.utt_off.ndim != 1 or len(self.utt_off) < 2 or self.utt_off[0] != 0 or self.utt_off[-1] != r
                or np.any(np.diff(self.utt_off) < 0)):
            raise ValueError("FrameDatabase: utt_off must run from 0 to %d without decreasing" % r)
        if kind == "lsf" and w // n_win != self.lsf_order:
            raise ValueError("FrameDatabase: %d static columns for order %d" % (w // n_win, self.lsf_order))
        self._dev = {}

    n_rows = property(lambda self: self.x.shape[0])
    width = property(lambda self: self.x.shape[1])
    n_static = property(lambda self: self.x.shape[1] // len(self.windows))
    n_utt = property(lambda self: len(self.utt_off) - 1)

    def variance_y(self):
        """The per-column variance of y over the rows (NumPy); 1.0 where it is zero or not finite."""
        with np.errstate(all="ignore"):
            v = np.var(self.y, axis=0)
        return np.where(np.isfinite(v) & (v > 0.0), v, 1.0)

    def host_tables(self):
        """What the kernels take, NumPy: 'x' and 'y' scaled (one rounded product per element), 'y_raw', 'succ', 'scale_x',
        'var_y'."""
        return {"x": self.x * self.scale_x, "y": self.y * self.scale_y, "y_raw": self.y, "succ": self.succ,
                "scale_x": self.scale_x, "var_y": self.variance_y()}

    def prepared(self, rt):
        """host_tables() resident on ``rt``'s device (uploaded once per runtime)."""
        key = (rt.index, rt.lane)
        if key not in self._dev:
            with rt.lock, rt.on_stream():
                t = self.host_tables()
                self._dev[key] = {k: rt.to_device(v, dtype=np.int32 if k == "succ" else np.float64) for k, v in t.items()}
        return self._dev[key]

    def exclusion(self, utterances):
        """(lo, hi) int32 per entry: the row range of that database utterance, or the empty range for None."""
        lo, hi = np.zeros(len(utterances), dtype=np.int32), np.zeros(len(utterances), dtype=np.int32)
        for i, u in enumerate(utterances):
            if u is None:
                continue
            if isinstance(u, bool) or int(u) != u or not 0 <= u < self.n_utt:
                raise ValueError("exclude: %r is no utterance of a database of %d" % (u, self.n_utt))
            lo[i], hi[i] = self.utt_off[int(u)], self.utt_off[int(u) + 1]
        return lo, hi

    def save_npz(self, path):
        out = {"x": self.x, "y": self.y, "succ": self.succ, "scale_x": self.scale_x, "scale_y": self.scale_y,
               "utt_off": self.utt_off, "windows": np.asarray(self.windows, dtype=np.float64), "kind": np.asarray(self.kind)}
        if self.kind == "lsf":
            out.update(lsf_order=np.asarray(self.lsf_order), lsf_min_gap=np.asarray(self.lsf_min_gap))
        np.savez(path, **out)

    @classmethod
    def load_npz(cls, path):
        with np.load(path) as z:
            kind = str(z["kind"])
            lsf = kind == "lsf"
            return cls(z["x"], z["y"], z["succ"], z["scale_x"], z["scale_y"], z["utt_off"],
                       tuple(tuple(w) for w in z["windows"]), kind, int(z["lsf_order"]) if lsf else None,
                       float(z["lsf_min_gap"]) if lsf else None)


def check_build_args(ce_a, ce_b, alignment, windows, where="build_compact"):
    """fit_compact's checks: ValueError before a device is touched.  Returns the static width."""
    from .gmm import check_lsf_width

    win, _ = check_windows(windows, where)
    for ce in (ce_a, ce_b):
        if ce.rt is None or (ce.mcep is None and ce.lsf is None):
            raise ValueError("%s: the encodings must be resident (to_device(rt)) and hold a mel-cepstrum or line spectral "
                             "frequencies" % where)
    if ce_a.kind != ce_b.kind or ce_a.lsf_order != ce_b.lsf_order:
        raise ValueError("%s: the two encodings differ in kind or order (%r %r against %r %r)"
                         % (where, ce_a.kind, ce_a.lsf_order, ce_b.kind, ce_b.lsf_order))
    if ce_a.fs != ce_b.fs:
        raise ValueError("%s: sampling rates differ (%r, %r): the rows would not be comparable" % (where, ce_a.fs, ce_b.fs))
    if ce_a.rt is not ce_b.rt:
        raise ValueError("%s: the two encodings live on different runtimes (device / lane)" % where)
    if ce_a.total_frames != alignment.batch_a.total_frames or ce_b.total_frames != alignment.batch_b.total_frames:
        raise ValueError("%s: the alignment was not made from these encodings (%d and %d frames against %d and %d)"
                         % (where, ce_a.total_frames, ce_b.total_frames, alignment.batch_a.total_frames,
                            alignment.batch_b.total_frames))
    if ce_b.total_frames < 1:
        raise ValueError("%s: the target has no frames" % where)
    rows = ce_a.lsf if ce_a.lsf is not None else ce_a.mcep
    rows_b = ce_b.lsf if ce_b.lsf is not None else ce_b.mcep
    d = int(rows.shape[1]) - 1
    if int(rows_b.shape[1]) - 1 != d or d < 1:
        raise ValueError("%s: rows of %d and %d coefficients" % (where, d + 1, int(rows_b.shape[1])))
    if ce_a.lsf is not None:
        check_lsf_width(ce_a.lsf_order, windows, where)
    if len(win) * d > MAX_D or d > MAX_DY:
        raise ValueError("%s: %d windows over %d columns; the kernels take rows of up to %d columns, %d of them static"
                         % (where, len(win), d, MAX_D, MAX_DY))
    return d


def _frames_batch(rt, frame_off):
    return rt.make_batch(np.zeros(len(frame_off), dtype=np.int64), frame_off)


# ---- device: the two calls on tensors ----------------------------------------------------------------------------------
def _rows(rt, name, t, where):
    if t.dim() != 2 or t.dtype != rt.torch.float64 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError("%s: %s must be a float64 [rows][d] tensor with unit column stride, got %s %s strides %s"
                         % (where, name, t.dtype, tuple(t.shape), tuple(t.stride())))
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


def knn_device(rt, q, db_rows, k, excl=None, splits=0):
    """wh_knn: for every row of q [n][d] the k rows of db_rows [R][d] that are nearest in squared distance, under the
    total order (distance, then row): (idx int32 [n][k], dist [n][k]), -1 / +inf in the slots beyond the candidates.
    ``excl``: (lo, hi), two int32 device tensors or arrays [n]: rows lo[n] <= r < hi[n] are no candidates of query n.
    ``splits``: 0, or the number of consecutive ranges the database is cut into (the same bytes for every value)."""
    torch = rt.torch
    ldq, lddb = _rows(rt, "q", q, "knn"), _rows(rt, "db_rows", db_rows, "knn")
    n, r = int(q.shape[0]), int(db_rows.shape[0])
    check_knn_args(n, int(q.shape[1]), r, int(db_rows.shape[1]), k, splits)
    d = int(q.shape[1])
    with rt.lock, rt.on_stream():
        lo = hi = None
        if excl is not None:
            lo, hi = (e if torch.is_tensor(e) else rt.to_device(np.ascontiguousarray(e, dtype=np.int32), dtype=np.int32)
                      for e in excl)
            for e in (lo, hi):
                if e.dtype != torch.int32 or tuple(e.shape) != (n,) or not e.is_contiguous():
                    raise ValueError("knn: the exclusion bounds must be contiguous int32 [%d]" % n)
        idx, dist = rt.empty((n, int(k)), torch.int32), rt.empty((n, int(k)))
        _hip.check(rt.lib.wh_knn(rt.ctx, rt.stream(), rt.ptr(q), n, max(ldq, d), rt.ptr(db_rows), r, max(lddb, d), d, int(k),
                                 rt.ptr(lo), rt.ptr(hi), int(splits), rt.ptr(idx), rt.ptr(dist)))
    return idx, dist


def select_device(rt, batch, idx, dist, y, succ, weight, want_acc=False):
    """wh_frame_select: one of every frame's candidates by Viterbi over every utterance of ``batch``: target cost dist,
    concatenation cost weight x the squared distance between y[candidate] and y[succ[the frame before's candidate]].
    Returns {'sel' int32 [frames]: the chosen database rows, 'slot' int32 [frames], 'total' [n_utt], 'acc' [frames][k]
    with want_acc}."""
    torch = rt.torch
    check_select_args(batch.total_frames, tuple(idx.shape), tuple(dist.shape), tuple(y.shape), int(succ.shape[0]), weight)
    ldy = _rows(rt, "y", y, "select")
    if idx.dtype != torch.int32 or succ.dtype != torch.int32 or dist.dtype != torch.float64:
        raise ValueError("select: idx and succ must be int32 and dist float64")
    if not (idx.is_contiguous() and dist.is_contiguous() and succ.is_contiguous()):
        raise ValueError("select: idx, dist and succ must be contiguous")
    frames, k, dy = batch.total_frames, int(idx.shape[1]), int(y.shape[1])
    with rt.lock, rt.on_stream():
        sel, slot = rt.empty((frames,), torch.int32), rt.empty((frames,), torch.int32)
        total = rt.empty((batch.n_utt,))
        acc = rt.empty((frames, k)) if want_acc else None
        _hip.check(rt.lib.wh_frame_select(rt.ctx, rt.stream(), batch.handle, rt.ptr(idx), rt.ptr(dist), k, rt.ptr(y),
                                          int(y.shape[0]), max(ldy, dy), dy, rt.ptr(succ), float(weight), rt.ptr(sel),
                                          rt.ptr(slot), rt.ptr(total), rt.ptr(acc)))
    out = {"sel": sel, "slot": slot, "total": total}
    if want_acc:
        out["acc"] = acc
    return out


# ---- rows [F][1 + d]: coefficient 0 / log E in front, as CompactEncoding keeps them ------------------------------------
def build_rows(rt, batch_a, rows_a, batch_b, rows_b, alignment, windows=CONVERSION_WINDOWS, normalise=True, kind="mcep",
               lsf_order=None):
    """FrameDatabase from the two speakers' rows and their Alignment: y the target's static + dynamic rows, x the source's
    gathered by alignment.map_b2a, both downloaded; the scales are computed on the host."""
    from .dynamics import delta_features_device
    from .gmm import lsf_min_gap

    gap = None
    with rt.lock, rt.on_stream():
        if kind == "lsf":
            gap = lsf_min_gap(rows_b)
            if not (gap > 0.0 and np.isfinite(gap)):
                raise ValueError("build_exemplars: the target's line spectral frequencies are not strictly ascending inside "
                                 "(0, pi) (smallest gap %r)" % gap)
        fa = delta_features_device(rt, batch_a, rows_a[:, 1:], windows)
        fb = delta_features_device(rt, batch_b, rows_b[:, 1:], windows)
        x = fa.index_select(0, alignment.map_b2a).cpu().numpy()
        y = fb.cpu().numpy()
    w = x.shape[1]
    scale_x = column_scales(x) if normalise else np.ones(w)
    scale_y = column_scales(y) if normalise else np.ones(w)
    utt_off = np.asarray(batch_b.frame_off, dtype=np.int64)
    return FrameDatabase(x, y, chain_succ(utt_off), scale_x, scale_y, utt_off, windows, kind, lsf_order, gap)


def check_convert_args(n_utt, d, db, k, weight, mode, exclude, where="convert"):
    """ValueError for what convert_rows cannot take, before a device is touched.  Returns the exclusion (lo, hi) per
    utterance, or None."""
    if mode not in MODES:
        raise ValueError("%s: mode must be one of %s, got %r" % (where, MODES, mode))
    if d != db.n_static:
        raise ValueError("%s: rows of %d coefficients against a database of %d" % (where, d + 1, db.n_static + 1))
    check_knn_args(0, db.width, db.n_rows, db.width, k, 0, where)
    if isinstance(weight, bool) or not (np.isfinite(weight) and weight >= 0.0):
        raise ValueError("%s: the weight must be finite and >= 0, got %r" % (where, weight))
    if exclude is None:
        return None
    exclude = list(exclude)
    if len(exclude) != n_utt:
        raise ValueError("%s: exclude has %d entries for %d utterances" % (where, len(exclude), n_utt))
    lo, hi = db.exclusion(exclude)
    if db.n_rows - int(np.max(hi - lo, initial=0)) < 1:
        raise ValueError("%s: the exclusion leaves no row of the database" % where)
    return lo, hi


def convert_rows(rt, batch, rows, db, k=16, weight=1.0, mode="frames", exclude=None, min_gap=None, splits=0):
    """Rows [F][1 + d] of ``batch`` -> (the converted rows, info).  The queries are the static + dynamic rows scaled by the
    database's scale_x; the concatenation cost is taken over the scaled static columns of y.  info: 'sel', 'slot', 'total',
    'idx' (device tensors)."""
    from .dynamics import delta_features_device, mlpg_device

    torch = rt.torch
    d = int(rows.shape[1]) - 1
    excl = check_convert_args(batch.n_utt, d, db, k, weight, mode, exclude)
    t = db.prepared(rt)
    with rt.lock, rt.on_stream():
        q = delta_features_device(rt, batch, rows[:, 1:], db.windows) * t["scale_x"]
        if excl is not None:
            reps = torch.from_numpy(np.diff(np.asarray(batch.frame_off, dtype=np.int64))).to(rt.device)
            excl = tuple(torch.repeat_interleave(rt.to_device(e, dtype=np.int32), reps).contiguous() for e in excl)
        idx, dist = knn_device(rt, q, t["x"], k, excl, splits)
        info = select_device(rt, batch, idx, dist, t["y"][:, :d], t["succ"], weight)
        info["idx"] = idx
        sel = info["sel"].to(torch.int64)
        if mode == "frames":
            out = torch.cat([rows[:, :1], t["y_raw"].index_select(0, sel)[:, :d]], dim=1)
        else:
            track = mlpg_device(rt, batch, t["y_raw"].index_select(0, sel), t["var_y"], db.windows)
            out = torch.cat([rows[:, :1], track], dim=1)
            if db.kind == "lsf":
                from .lsf import repair_device
                repair_device(rt, out[:, 1:], db.lsf_min_gap if min_gap is None else min_gap, out=out[:, 1:])
    return out, info


# ---- CompactEncoding -------------------------------------------------------------------------------------------------
def build_compact(ce_a, ce_b, alignment, windows=CONVERSION_WINDOWS, normalise=True):
    """FrameDatabase for two resident CompactEncodings of parallel utterances and their Alignment: row r is target frame
    r of ``ce_b`` (batch-global)."""
    check_build_args(ce_a, ce_b, alignment, windows)
    rt = ce_a.rt
    key = "lsf" if ce_a.lsf is not None else "mcep"
    with rt.lock, rt.on_stream():
        return build_rows(rt, _frames_batch(rt, ce_a.frame_off), getattr(ce_a, key), _frames_batch(rt, ce_b.frame_off),
                          getattr(ce_b, key), alignment, windows, normalise, key, ce_a.lsf_order if key == "lsf" else None)


def convert_compact(ce, db, k=16, weight=1.0, mode="frames", exclude=None, min_gap=None):
    """(CompactEncoding, info): ``ce``'s mel-cepstral columns 1 .. n0-1 (or its p angles) replaced by frame selection from
    ``db``; coefficient 0 / log E, f0, vuv, band aperiodicity, the voicing gate and the frame times are carried over, as
    gmm.convert_compact carries them.  mode 'frames': the static columns of the selected target rows, bit for bit rows of
    the database.  'mlpg': the selected static + dynamic rows as means and the database's per-column variance, through
    mlpg_device (and, for line spectral frequencies, the repair).  ``exclude``: per utterance a database utterance index
    or None — leave-one-out conversion of a training utterance."""
    if ce.rt is None:
        raise ValueError("convert_compact: the encoding is on the host; to_device(rt) first")
    if ce.mcep is None and ce.lsf is None:
        raise ValueError("convert_compact: the encoding keeps the dense spectrogram (compact(n0=None)): no mel-cepstrum")
    if ce.kind != db.kind or ce.lsf_order != db.lsf_order:
        raise ValueError("convert_compact: an encoding of kind %r, order %r against a database of kind %r, order %r"
                         % (ce.kind, ce.lsf_order, db.kind, db.lsf_order))
    key = "lsf" if ce.lsf is not None else "mcep"
    rows = getattr(ce, key)
    check_convert_args(ce.n_utt, int(rows.shape[1]) - 1, db, k, weight, mode, exclude, "convert_compact")
    rt = ce.rt
    with rt.lock, rt.on_stream():
        arrays = dict(ce._tensors())
        arrays[key], info = convert_rows(rt, _frames_batch(rt, ce.frame_off), rows, db, k, weight, mode, exclude, min_gap)
    return ce._like(rt, arrays, None if ce.tp_host is None else np.array(ce.tp_host)), info


def convert_waveform(wb, batch, x_d, ce, db, hop=None, **kw):
    """Vocoder-free conversion by frame selection: convert_compact(ce, db, **kw), then the recording ``x_d`` of ``batch``
    filtered by the converted over the source envelope (world.specfilter.differential_device), as gmm.convert_waveform.
    Returns (y_d in x's layout, the converted CompactEncoding, info).  The f0 stays the recording's: to move it first,
    world.psola.modify_device(.., pitch=world.tsm.log_f0_ratio(a, b)) leaves the formants in place."""
    from .specfilter import differential_device

    converted, info = convert_compact(ce, db, **kw)
    return differential_device(wb, batch, x_d, ce, converted, hop=hop), converted, info


# ---- NumPy-dict forms (World.build_exemplars / convert_voice_exemplar) -------------------------------------------------
def _dict_rows(rt, enc, kind, n0, lsf_order, lowhz, highhz):
    if kind == "lsf":
        from .lsf import lsf_device
        return lsf_device(rt, enc.spectrogram, lsf_order)
    return enc.mcep(n0, lowhz, highhz)


def build_exemplars_dicts(dats_a, dats_b, n0=40, lsf_order=None, radius=None, lowhz=0, highhz=8000,
                          windows=CONVERSION_WINDOWS, normalise=True):
    """World.build_exemplars: align the pairs, return the FrameDatabase."""
    from .align import align_device, check_radius
    from .batch import BatchEncoding

    dats_a, dats_b = list(dats_a), list(dats_b)
    if len(dats_a) != len(dats_b) or not dats_a:
        raise ValueError("build_exemplars: %d dict(s) against %d: pair u is dict u of each side" % (len(dats_a), len(dats_b)))
    win, _ = check_windows(windows, "build_exemplars")
    check_radius(radius, "build_exemplars")
    rates = {d['fs'] for d in dats_a} | {d['fs'] for d in dats_b}
    if len(rates) != 1:
        raise ValueError("build_exemplars: sampling rates differ (%s): the rows would not be comparable" % sorted(rates))
    if lsf_order is not None:
        from .gmm import check_lsf_width
        from .lsf import check_order
        kind, d = "lsf", check_order(lsf_order, "build_exemplars")
        check_lsf_width(d, windows, "build_exemplars")
    else:
        if isinstance(n0, bool) or int(n0) != n0 or n0 < 2:
            raise ValueError("build_exemplars: n0 must be an integer >= 2, got %r" % (n0,))
        kind, d = "mcep", int(n0) - 1
    if len(win) * d > MAX_D or d > MAX_DY:
        raise ValueError("build_exemplars: %d windows over %d columns; the kernels take rows of up to %d columns, %d of them "
                         "static" % (len(win), d, MAX_D, MAX_DY))
    rt = _hip.Runtime.get()
    with rt.lock, rt.on_stream():
        enc_a, enc_b = BatchEncoding.from_dicts(rt, dats_a), BatchEncoding.from_dicts(rt, dats_b)
        ra = _dict_rows(rt, enc_a, kind, n0, lsf_order, lowhz, highhz)
        rb = _dict_rows(rt, enc_b, kind, n0, lsf_order, lowhz, highhz)
        al = align_device(rt, enc_a.batch, ra[:, 1:], enc_b.batch, rb[:, 1:], radius)
        db = build_rows(rt, enc_a.batch, ra, enc_b.batch, rb, al, windows, normalise, kind,
                        int(lsf_order) if kind == "lsf" else None)
    rt.check_flags("build_exemplars")
    return db


def convert_voice_exemplar_dict(dat, db, k=16, weight=1.0, mode="frames", lowhz=0, highhz=8000):
    """World.convert_voice_exemplar: a new dict like ``dat`` whose 'spectrogram' is rebuilt from the converted rows."""
    from .batch import BatchEncoding

    fft_size = 2 * (int(np.shape(dat['spectrogram'])[0]) - 1)
    n0 = db.n_static + 1
    check_convert_args(1, db.n_static, db, k, weight, mode, None, "convert_voice_exemplar")
    if db.kind != "lsf":
        from .compact import check_compact_args
        check_compact_args(dat['fs'], fft_size, n0, "convert_voice_exemplar")
    rt = _hip.Runtime.get()
    with rt.lock, rt.on_stream():
        enc = BatchEncoding.from_dicts(rt, [dat])
        rows = _dict_rows(rt, enc, db.kind, n0, db.lsf_order, lowhz, highhz)
        conv, _ = convert_rows(rt, enc.batch, rows, db, k, weight, mode)
        if db.kind == "lsf":
            from .lsf import ilsf_device
            spec = rt.to_host(ilsf_device(rt, conv, fft_size), transpose=True)
        else:
            from .features import imcep_device
            spec = rt.to_host(imcep_device(rt, conv, fft_size), transpose=True)
    rt.check_flags("convert_voice_exemplar")
    out = {k_: (np.array(v) if isinstance(v, np.ndarray) else v) for k_, v in dict(dat).items() if k_ != 'out'}
    out['spectrogram'] = np.ascontiguousarray(spec)
    return out
