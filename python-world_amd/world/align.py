"""Frame alignment of parallel utterances by dynamic time warping over feature rows (mel-cepstra): the step in front of
a voice-conversion mapping between two speakers' recordings of the same sentences (the reference ships such
conversions under manifold/samples/{F2F,F2M,M2F,M2M} and no code for them), of the aligned mel-cepstral distortion, and
of putting one speaker's spectra on another speaker's timing.  The kernels are behind wh_dtw (csrc/wh_dtw.hip); the
arithmetic is a contract (include/world_hip.h) that tests/_dtw_reference.py states in NumPy and the
device reproduces bit for bit.

The argument checks, the workspace grouping and the map rule are host code and need neither the library nor a GPU."""
import ctypes

import numpy as np

from . import _hip

# the recurrence kernel's tiling (csrc/wh_dtw.hip: kDtwRowsPerLane, kDtwStripRows, kDtwChunkCols); the tests put their
# shapes around these, and tests/test_align_host.py holds the two files together
ROWS_PER_LANE = 2
STRIP_ROWS = 64 * ROWS_PER_LANE
CHUNK_COLS = 32
MAX_D = 64
DEFAULT_MAX_WORKSPACE_BYTES = 4 << 30
MCD_SCALE = (10.0 / np.log(10.0)) * np.sqrt(2.0)  # dB per unit of mean cost (Kubichek's mel-cepstral distortion)


# ---- host ----------------------------------------------------------------------------------------------------------
def pair_workspace_bytes(n, m):
    """What one pair of n x m frames takes of the context's scratch while it is aligned: two bits per cell in rows padded
    to 16 cells, and one line of m doubles between the strips — 4 n ceil(m / 16) + 8 m bytes (1.0 MB for 2001 x 2001)."""
    return 4 * int(n) * ((int(m) + 15) // 16) + 8 * int(m)


def plan_groups(na, nb, max_workspace_bytes=DEFAULT_MAX_WORKSPACE_BYTES):
    """Consecutive pairs [u0, u1) per wh_dtw call: as many as fit ``max_workspace_bytes`` of back-pointer workspace,
    taken in order; a pair that is larger than the limit on its own is a group of one."""
    groups, u0, used = [], 0, 0
    for u, (n, m) in enumerate(zip(na, nb)):
        need = pair_workspace_bytes(n, m)
        if u > u0 and used + need > max_workspace_bytes:
            groups.append((u0, u))
            u0, used = u, 0
        used += need
    if len(na) > u0:
        groups.append((u0, len(na)))
    return groups


def check_radius(radius, where="align"):
    if radius is None:
        return 0
    if isinstance(radius, bool) or int(radius) != radius or radius < 1:
        raise ValueError("%s: radius must be None or an integer >= 1, got %r" % (where, radius))
    return int(radius)


def check_pair_shapes(frame_off_a, frame_off_b, d, where="align"):
    """ValueError for what wh_dtw refuses, before anything reaches the device.  Returns the two frame-count arrays."""
    if len(frame_off_a) != len(frame_off_b):
        raise ValueError("%s: %d utterance(s) against %d: pair u aligns utterance u of each side"
                         % (where, len(frame_off_a) - 1, len(frame_off_b) - 1))
    if not 1 <= d <= MAX_D:
        raise ValueError("%s: rows of %d columns; the kernel keeps a row in registers and takes 1 .. %d" % (where, d, MAX_D))
    na, nb = np.diff(np.asarray(frame_off_a, dtype=np.int64)), np.diff(np.asarray(frame_off_b, dtype=np.int64))
    for side, n in (("first", na), ("second", nb)):
        if np.any(n < 1):
            raise ValueError("%s: utterance %d of the %s batch has no frames" % (where, int(np.argmax(n < 1)), side))
    return na, nb


def maps_from_path(path_a, path_b, n, m):
    """The frame maps of a path (pair-local indices): map_a2b[i] = (j_lo + j_hi) // 2 over the path cells that share i,
    map_b2a[j] likewise over those that share j."""
    path_a, path_b = np.asarray(path_a, dtype=np.int64), np.asarray(path_b, dtype=np.int64)

    def one(key, val, size):
        lo = np.full(size, np.iinfo(np.int64).max, dtype=np.int64)
        hi = np.full(size, -1, dtype=np.int64)
        np.minimum.at(lo, key, val)
        np.maximum.at(hi, key, val)
        return (lo + hi) // 2

    return one(path_a, path_b, int(n)), one(path_b, path_a, int(m))


def check_encodings(enc_a, enc_b, n0, where="align"):
    """BatchEncoding.align's checks: ValueError before the device is touched."""
    if enc_a.rt is not enc_b.rt:
        raise ValueError("%s: the two encodings live on different runtimes (device / lane)" % where)
    if enc_a.fs != enc_b.fs:
        raise ValueError("%s: sampling rates differ (%r, %r): the mel-cepstra would not be comparable" % (where, enc_a.fs, enc_b.fs))
    if enc_a.n_utt != enc_b.n_utt:
        raise ValueError("%s: %d utterance(s) against %d: pair u aligns utterance u of each side"
                         % (where, enc_a.n_utt, enc_b.n_utt))
    if int(n0) != n0 or n0 < 2 or n0 - 1 > MAX_D:
        raise ValueError("%s: n0 must be an integer in [2, %d] (coefficient 0, the energy, is dropped and the kernel takes "
                         "rows of up to %d columns), got %r" % (where, MAX_D + 1, MAX_D, n0))


# ---- device --------------------------------------------------------------------------------------------------------
class Alignment:
    """The result of align_device, resident.  Pair u's path is entries path_off[u] .. path_off[u] + path_len[u] of
    ``path_a`` / ``path_b`` (int64, frame indices into the whole batch on each side, as torch.index_select takes them;
    each pair has room for N + M - 1 entries and what lies behind its length is unspecified); ``cost`` [n_utt] is
    D(N-1, M-1), the sum of the local costs along the path; ``map_a2b`` [frames of a] and ``map_b2a`` [frames of b] give
    for every frame the frame of the other side at the middle of its run on the path.  ``path_off`` is a device tensor,
    ``path_off_host`` its NumPy twin.  ``acc`` (want_acc=True) holds D of every pair, row-major, at ``acc_off_host``."""

    def __init__(self, rt, batch_a, batch_b, path_a, path_b, path_off_host, path_len, cost, map_a2b, map_b2a, acc=None,
                 acc_off_host=None):
        self.rt, self.batch_a, self.batch_b = rt, batch_a, batch_b
        self.path_a, self.path_b, self.path_len, self.cost = path_a, path_b, path_len, cost
        self.map_a2b, self.map_b2a = map_a2b, map_b2a
        self.path_off_host = path_off_host
        self.path_off = rt.torch.from_numpy(path_off_host).to(rt.device)
        self.acc, self.acc_off_host = acc, acc_off_host
        self._len_host = None

    @property
    def n_utt(self):
        return self.batch_a.n_utt

    def lengths(self):
        """Path lengths on the host (downloaded once)."""
        if self._len_host is None:
            self._len_host = self.path_len.cpu().numpy()
        return self._len_host

    def mean_cost(self):
        """cost / path length per pair: device tensor [n_utt]."""
        return self.cost / self.path_len.to(self.cost.dtype)

    def mcd_db(self):
        """(10 / ln 10) sqrt(2) mean_cost per pair — the mel-cepstral distortion in dB when the rows are mel-cepstral
        coefficients 1 .. n0-1."""
        return self.mean_cost() * MCD_SCALE

    def lsd_db(self, rows_a, rows_b, fft_size, gain=False):
        """The aligned log-spectral distortion in dB per pair, device tensor [n_utt]: the mean over the pair's path of
        world.lsf.distortion_device between row path_a of ``rows_a`` and row path_b of ``rows_b`` — rows
        [log E, w_1 .. w_p] of line spectral frequencies over the frames of the two batches (the aligned ones, or any
        others on the same frames: a conversion scored against its target).  ``gain=False``: the distortion of the
        spectral shape, the best constant gain taken out of every cell.  What mcd_db() is to mel-cepstral rows."""
        from .lsf import distortion_device

        rt, torch = self.rt, self.rt.torch
        for name, rows, batch in (("rows_a", rows_a, self.batch_a), ("rows_b", rows_b, self.batch_b)):
            if rows.dim() != 2 or int(rows.shape[0]) != batch.total_frames:
                raise ValueError("lsd_db: %s must be [%d frames][p + 1], got %s" % (name, batch.total_frames, tuple(rows.shape)))
        with rt.lock, rt.on_stream():
            pos, off = self.valid_index()
            d = distortion_device(rt, rows_a, rows_b, fft_size, self.path_a.index_select(0, pos),
                                  self.path_b.index_select(0, pos), gain)
            lengths = torch.from_numpy(np.diff(off)).to(rt.device)
            return torch.segment_reduce(d, "mean", lengths=lengths)

    def pairs(self, u):
        """(i, j): pair u's path as two host arrays of utterance-local frame indices."""
        o, n = int(self.path_off_host[u]), int(self.lengths()[u])
        pa, pb = self.rt.torch.stack([self.path_a[o:o + n], self.path_b[o:o + n]]).cpu().numpy()
        return pa - int(self.batch_a.frame_off[u]), pb - int(self.batch_b.frame_off[u])

    def valid_index(self):
        """Positions of the paths' entries in path_a / path_b, pair after pair (device int64), and their offsets (host)."""
        torch = self.rt.torch
        ln = self.lengths()
        off = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
        pos = np.concatenate([np.arange(o, o + n, dtype=np.int64) for o, n in zip(self.path_off_host[:-1], ln)]
                             or [np.zeros(0, dtype=np.int64)])
        return torch.from_numpy(pos).to(self.rt.device), off

    def joint(self, xa, xb):
        """The aligned rows side by side: a tensor [sum of path lengths][da + db], row p of pair u being
        xa[path_a] | xb[path_b] at path position p — the joint vectors a conversion model is trained on — and the host
        offsets [n_utt + 1] of the pairs in it."""
        pos, off = self.valid_index()
        ra = xa.index_select(0, self.path_a.index_select(0, pos))
        rb = xb.index_select(0, self.path_b.index_select(0, pos))
        return self.rt.torch.cat([ra, rb], dim=1), off

    def warp(self, enc_a, enc_b):
        """``enc_a`` on ``enc_b``'s timing: a new BatchEncoding on enc_b's batch descriptor and frame times whose rows are
        enc_a's rows gathered by map_b2a — f0, vuv, spectrogram, aperiodicity, and coarse_ap / ap_gate when present.  The
        source speaker at the target's pace, ready for decode_device, compact() and the feature heads.  It carries no
        'ps spectrogram' and no prefetched time base."""
        from .batch import BatchEncoding

        if enc_a.batch.total_frames != self.batch_a.total_frames or enc_b.batch.total_frames != self.batch_b.total_frames:
            raise ValueError("warp: the encodings are not the ones this alignment was made from (%d and %d frames against "
                             "%d and %d)" % (enc_a.batch.total_frames, enc_b.batch.total_frames, self.batch_a.total_frames,
                                             self.batch_b.total_frames))
        rt = self.rt
        with rt.lock, rt.on_stream():
            take = lambda t: None if t is None else t.index_select(0, self.map_b2a)  # noqa: E731
            out = BatchEncoding(rt, enc_b.batch, enc_a.fs, enc_b.temporal_positions.clone(), take(enc_a.f0), take(enc_a.vuv),
                                take(enc_a.spectrogram), take(enc_a.aperiodicity), enc_a.fft_size, enc_a.is_requiem,
                                enc_b.frame_period, tp_host=None if enc_b.tp_host is None else enc_b.tp_host.copy())
            out.coarse_ap, out.ap_gate = take(enc_a.coarse_ap), take(enc_a.ap_gate)
        return out


def _sub_batch(rt, batch, u0, u1):
    fo = batch.frame_off[u0:u1 + 1] - batch.frame_off[u0]
    return rt.make_batch(np.zeros(u1 - u0 + 1, dtype=np.int64), fo)


def align_device(rt, batch_a, xa, batch_b, xb, radius=None, want_acc=False,
                 max_workspace_bytes=DEFAULT_MAX_WORKSPACE_BYTES):
    """Dynamic time warping of every pair (utterance u of ``batch_a`` over xa, utterance u of ``batch_b`` over xb) on the
    device.  xa / xb: float64 device tensors [frames][d] with unit column stride (a column slice of a wider tensor is
    fine: the row stride is passed on), 1 <= d <= 64.  ``radius``: None for the whole rectangle, or the band
    |j (N-1) - i (M-1)| <= radius max(N-1, M-1).  ``want_acc``: also keep the accumulated-cost matrices (8 N M bytes per
    pair: a test hook for small shapes).  The back-pointers take pair_workspace_bytes(N, M) of the context's scratch per
    pair — two bits per cell — and the pairs are handed to the kernel in consecutive groups (plan_groups) that keep that
    under ``max_workspace_bytes``; a pair's result does not depend on its group.  Returns an Alignment."""
    torch = rt.torch
    for name, x, batch in (("xa", xa, batch_a), ("xb", xb, batch_b)):
        if x.dim() != 2 or x.dtype != torch.float64 or x.stride(1) != 1 or int(x.shape[0]) != batch.total_frames:
            raise ValueError("align: %s must be a float64 [%d frames][d] tensor with unit column stride, got %s %s strides %s"
                             % (name, batch.total_frames, x.dtype, tuple(x.shape), tuple(x.stride())))
    if xa.shape[1] != xb.shape[1]:
        raise ValueError("align: rows of %d and of %d columns" % (xa.shape[1], xb.shape[1]))
    d = int(xa.shape[1])
    na, nb = check_pair_shapes(batch_a.frame_off, batch_b.frame_off, d)
    r = check_radius(radius)
    n_utt = batch_a.n_utt
    path_off = np.concatenate([[0], np.cumsum(na + nb - 1)]).astype(np.int64)
    acc_off = np.concatenate([[0], np.cumsum(na * nb)]).astype(np.int64) if want_acc else None
    groups = plan_groups(na, nb, max_workspace_bytes)
    i64 = torch.int64
    with rt.lock, rt.on_stream():
        path_a, path_b = rt.empty((int(path_off[-1]),), i64), rt.empty((int(path_off[-1]),), i64)
        path_len, cost = rt.empty((n_utt,), i64), rt.empty((n_utt,))
        map_a2b, map_b2a = rt.empty((batch_a.total_frames,), i64), rt.empty((batch_b.total_frames,), i64)
        acc = rt.empty((int(acc_off[-1]),)) if want_acc else None
        foa, fob = batch_a.frame_off, batch_b.frame_off
        for u0, u1 in groups:
            whole = (u0, u1) == (0, n_utt)
            ga = batch_a if whole else _sub_batch(rt, batch_a, u0, u1)
            gb = batch_b if whole else _sub_batch(rt, batch_b, u0, u1)
            a0, a1, b0, b1 = int(foa[u0]), int(foa[u1]), int(fob[u0]), int(fob[u1])
            p0, p1 = int(path_off[u0]), int(path_off[u1])
            g_path_off = np.ascontiguousarray(path_off[u0:u1 + 1] - p0)
            g_acc_off = np.ascontiguousarray(acc_off[u0:u1 + 1] - acc_off[u0]) if want_acc else None
            g_acc = acc[int(acc_off[u0]):int(acc_off[u1])] if want_acc else None
            xa_g, xb_g = xa[a0:a1], xb[b0:b1]
            _hip.check(rt.lib.wh_dtw(rt.ctx, rt.stream(), ga.handle, gb.handle, rt.ptr(xa_g), int(xa.stride(0)),
                                     rt.ptr(xb_g), int(xb.stride(0)), d, r, g_path_off.ctypes.data_as(_hip._c_i64p),
                                     rt.ptr(path_a[p0:p1]), rt.ptr(path_b[p0:p1]), rt.ptr(path_len[u0:u1]),
                                     rt.ptr(cost[u0:u1]), rt.ptr(map_a2b[a0:a1]), rt.ptr(map_b2a[b0:b1]), rt.ptr(g_acc),
                                     g_acc_off.ctypes.data_as(_hip._c_i64p) if want_acc else None))
            if not whole:  # the group's indices count from its own first frame
                path_a[p0:p1] += a0
                path_b[p0:p1] += b0
                map_a2b[a0:a1] += b0
                map_b2a[b0:b1] += a0
    return Alignment(rt, batch_a, batch_b, path_a, path_b, path_off, path_len, cost, map_a2b, map_b2a, acc, acc_off)


def align_encodings(enc_a, enc_b, n0=40, lowhz=0, highhz=8000, radius=None,
                    max_workspace_bytes=DEFAULT_MAX_WORKSPACE_BYTES):
    """BatchEncoding.align: see there."""
    check_encodings(enc_a, enc_b, n0)
    check_radius(radius)
    check_pair_shapes(enc_a.batch.frame_off, enc_b.batch.frame_off, int(n0) - 1)
    rt = enc_a.rt
    with rt.lock, rt.on_stream():
        ma, mb = enc_a.mcep(n0, lowhz, highhz), enc_b.mcep(n0, lowhz, highhz)
        return align_device(rt, enc_a.batch, ma[:, 1:], enc_b.batch, mb[:, 1:], radius,
                            max_workspace_bytes=max_workspace_bytes)


def check_compact_pair(ce_a, ce_b, where="align_compact"):
    """ValueError unless the two CompactEncodings can be compared row by row: the same kind ('mcep' or 'lsf'), the same
    number of coefficients and the same sampling rate.  Touches no device.  Returns the number of columns compared."""
    if ce_a.kind != ce_b.kind or ce_a.kind == "spectrogram":
        raise ValueError("%s: encodings of kind %r and %r: both must hold a mel-cepstrum, or both line spectral frequencies"
                         % (where, ce_a.kind, ce_b.kind))
    if ce_a.fs != ce_b.fs:
        raise ValueError("%s: sampling rates differ (%r, %r): the rows would not be comparable" % (where, ce_a.fs, ce_b.fs))
    if ce_a.kind == "lsf":
        if ce_a.lsf_order != ce_b.lsf_order:
            raise ValueError("%s: line spectral frequencies of order %d and %d" % (where, ce_a.lsf_order, ce_b.lsf_order))
        return ce_a.lsf_order
    if ce_a.n0 != ce_b.n0 or ce_a.mcep_fs != ce_b.mcep_fs:
        raise ValueError("%s: mel-cepstra of %r coefficients at %r Hz and of %r at %r Hz"
                         % (where, ce_a.n0, ce_a.mcep_fs, ce_b.n0, ce_b.mcep_fs))
    return int(ce_a.n0) - 1


def align_compact(ce_a, ce_b, radius=None, max_workspace_bytes=DEFAULT_MAX_WORKSPACE_BYTES):
    """CompactEncoding.align: dynamic time warping of utterance u of ``ce_a`` against utterance u of ``ce_b`` over the
    stored rows — mcep[:, 1:], or the p angles lsf[:, 1:]; coefficient 0 / the gain is dropped — so a corpus kept as
    compact .npz files is aligned without its spectrograms.  Both encodings resident on one runtime.  Returns an Alignment."""
    d = check_compact_pair(ce_a, ce_b)
    if ce_a.rt is None or ce_b.rt is None:
        raise ValueError("align_compact: the encodings must be resident (to_device(rt))")
    if ce_a.rt is not ce_b.rt:
        raise ValueError("align_compact: the two encodings live on different runtimes (device / lane)")
    check_radius(radius)
    check_pair_shapes(ce_a.frame_off, ce_b.frame_off, d, "align_compact")
    rt = ce_a.rt
    key = ce_a.kind
    with rt.lock, rt.on_stream():
        zeros = np.zeros(ce_a.n_utt + 1, dtype=np.int64)
        return align_device(rt, rt.make_batch(zeros, ce_a.frame_off), getattr(ce_a, key)[:, 1:],
                            rt.make_batch(zeros, ce_b.frame_off), getattr(ce_b, key)[:, 1:], radius,
                            max_workspace_bytes=max_workspace_bytes)


# ---- NumPy-dict forms (World.align / align_batch / warp_to) ---------------------------------------------------------
def align_dicts(dats_a, dats_b, n0=40, lowhz=0, highhz=8000, radius=None):
    """World.align_batch: one result dict per pair."""
    from .batch import BatchEncoding

    dats_a, dats_b = list(dats_a), list(dats_b)
    if len(dats_a) != len(dats_b):
        raise ValueError("align: %d dict(s) against %d: pair u aligns dict u of each side" % (len(dats_a), len(dats_b)))
    if not dats_a:
        return []
    fs = {d['fs'] for d in dats_a} | {d['fs'] for d in dats_b}
    if len(fs) != 1:
        raise ValueError("align: sampling rates differ (%s): the mel-cepstra would not be comparable" % sorted(fs))
    if int(n0) != n0 or n0 < 2 or n0 - 1 > MAX_D:
        raise ValueError("align: n0 must be an integer in [2, %d], got %r" % (MAX_D + 1, n0))
    check_radius(radius)
    for side, dats in (("first", dats_a), ("second", dats_b)):
        for u, d in enumerate(dats):
            if len(d['f0']) < 1:
                raise ValueError("align: dict %d of the %s list has no frames" % (u, side))
    rt = _hip.Runtime.get()
    with rt.lock:
        al = align_encodings(BatchEncoding.from_dicts(rt, dats_a), BatchEncoding.from_dicts(rt, dats_b), n0, lowhz, highhz,
                             radius)
        with rt.on_stream():
            cost, mcd = rt.torch.stack([al.cost, al.mcd_db()]).cpu().numpy()
        out = []
        for u in range(al.n_utt):
            pa, pb = al.pairs(u)
            out.append({'path_a': pa, 'path_b': pb, 'cost': float(cost[u]), 'mcd': float(mcd[u])})
    return out


def warp_dict(dat_a, dat_b, alignment):
    """World.warp_to: dat_a's frames on dat_b's timing, by the map rule on the alignment's path."""
    na, nb = len(dat_a['f0']), len(dat_b['f0'])
    pa, pb = np.asarray(alignment['path_a'], dtype=np.int64), np.asarray(alignment['path_b'], dtype=np.int64)
    if len(pa) != len(pb) or len(pa) == 0 or pa[0] != 0 or pb[0] != 0 or pa[-1] != na - 1 or pb[-1] != nb - 1:
        raise ValueError("warp_to: the path does not run from (0, 0) to (%d, %d): not an alignment of these two dicts"
                         % (na - 1, nb - 1))
    _, b2a = maps_from_path(pa, pb, na, nb)
    out = {'temporal_positions': np.array(dat_b['temporal_positions'], dtype=np.float64), 'fs': dat_a['fs'],
           'is_requiem': dat_a['is_requiem'], 'f0': np.asarray(dat_a['f0'])[b2a], 'vuv': np.asarray(dat_a['vuv'])[b2a],
           'spectrogram': np.ascontiguousarray(np.asarray(dat_a['spectrogram'])[:, b2a]),
           'aperiodicity': np.ascontiguousarray(np.asarray(dat_a['aperiodicity'])[:, b2a])}
    return out
