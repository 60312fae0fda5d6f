"""Inputs, NumPy references and drivers shared by tests/test_hip_regrid.py, tests/test_hip_contour.py and
tests/_regrid_bounds_script.py: wh_regrid_rows and wh_interp_contour called directly on made tensors.  The oracle is
np.interp itself, per utterance and per bin; the both-bracketing rule is restated here in NumPy, independently of
world/regrid.py."""
import ctypes

import numpy as np

_vp = ctypes.c_void_p
SHAPE_K = (1, 2, 5, 513, 1025)
SHAPE_FRAMES = (1, 2, 3, 401)


def offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def make_batch(rt, counts):
    return rt.make_batch(np.zeros(len(counts) + 1, dtype=np.int64), offsets(counts))


def shifted(rt, a, shift):
    """``a`` on the device as a view ``shift`` elements into a larger tensor: shift 1 puts its base off a 16-byte boundary."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    big = rt.empty((a.size + 2,))
    assert big.data_ptr() % 16 == 0
    view = big[shift:shift + a.size].view(a.shape)
    view.copy_(rt.torch.from_numpy(a))
    return view


# ---- NumPy statements of what the kernels compute ---------------------------------------------------------------------
def read_knots(xp, x):
    """The knots np.interp reads for the queries x: (first index, second index), equal where it reads one — below the
    first knot, above the last, on the last, on an exact hit."""
    xp, x = np.asarray(xp), np.asarray(x)
    n = len(xp)
    j = np.clip(np.searchsorted(xp, x, side="right") - 1, 0, n - 1)
    one = (x < xp[0]) | (x > xp[-1]) | (j == n - 1) | (xp[j] == x)
    return j, np.where(one, j, np.minimum(j + 1, n - 1))


def ref_rows(tp_src, tp_dst, rows, positive=False):
    """np.interp per bin for one utterance; ``positive``: 0 unless every source value read is > 0."""
    rows = np.asarray(rows, dtype=np.float64).reshape(len(tp_src), -1)
    out = np.stack([np.interp(tp_dst, tp_src, rows[:, k]) for k in range(rows.shape[1])], axis=1)
    if positive:
        j0, j1 = read_knots(tp_src, tp_dst)
        out = np.where((rows[j0] > 0) & (rows[j1] > 0), out, 0.0)
    return out


def ref_batch(src_parts, dst_parts, rows, positive=False):
    so = offsets([len(p) for p in src_parts])
    return np.concatenate([ref_rows(s, d, rows[so[u]:so[u + 1]], positive)
                           for u, (s, d) in enumerate(zip(src_parts, dst_parts))])


def regrid(rt, src_parts, dst_parts, rows, positive=False, in_shift=0, out_shift=0):
    """wh_regrid_rows on host arrays: rows [F][K] (or [F]) -> NumPy [F'][K]; the base pointers as the shifts say."""
    from world import _hip

    rows = np.asarray(rows, dtype=np.float64)
    k = 1 if rows.ndim == 1 else rows.shape[1]
    sb, db = make_batch(rt, [len(p) for p in src_parts]), make_batch(rt, [len(p) for p in dst_parts])
    n_dst = db.total_frames
    in_d = shifted(rt, rows, in_shift)
    out_d = shifted(rt, np.full((n_dst, k), -7.0), out_shift)
    assert out_d.data_ptr() % 16 == 8 * out_shift and in_d.data_ptr() % 16 == 8 * in_shift
    tp_s, tp_d = rt.to_device(np.concatenate(src_parts)), rt.to_device(np.concatenate(dst_parts))
    _hip.check(rt.lib.wh_regrid_rows(rt.ctx, rt.stream(), sb.handle, db.handle, rt.ptr(tp_s), rt.ptr(tp_d), rt.ptr(in_d),
                                     rt.ptr(out_d), int(k), 1 if positive else 0))
    return out_d.cpu().numpy()


def contour(rt, tp_parts, knots, voiced_rule):
    """wh_interp_contour on host arrays: knots = [(time, value)] per utterance -> (out, vuv or None) as NumPy."""
    from world import _hip

    b = make_batch(rt, [len(p) for p in tp_parts])
    off = offsets([len(t) for t, _ in knots])
    kt = np.ascontiguousarray(np.concatenate([t for t, _ in knots]), dtype=np.float64)
    kv = np.ascontiguousarray(np.concatenate([v for _, v in knots]), dtype=np.float64)
    out = rt.empty((b.total_frames,))
    vuv = rt.empty((b.total_frames,)) if voiced_rule else None
    tp_d = rt.to_device(np.concatenate(tp_parts))
    _hip.check(rt.lib.wh_interp_contour(rt.ctx, rt.stream(), b.handle, rt.ptr(tp_d),
                                        off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), kt.ctypes.data_as(_vp),
                                        kv.ctypes.data_as(_vp), 1 if voiced_rule else 0, rt.ptr(out), rt.ptr(vuv)))
    return out.cpu().numpy(), None if vuv is None else vuv.cpu().numpy()


# ---- inputs ------------------------------------------------------------------------------------------------------------
def shape_case(k_bins, seed=0):
    """Utterances of 1, 2, 3 and 401 frames on a jittered 5 ms grid; destination times below the first source frame,
    above the last, exactly on source frames and in between.  With an odd K the number of output elements is odd (the
    lone last bin of the pair walk)."""
    rng = np.random.RandomState(100 + seed)
    src, dst = [], []
    for n in SHAPE_FRAMES:
        t = np.arange(n) * 0.005 + rng.uniform(-0.001, 0.001, n) + 0.01
        g = np.arange(-0.004, t[-1] - t[0] + 0.009, 0.0037) + t[0]
        d = np.unique(np.concatenate([g, t[::3], [t[-1]]]))
        src.append(t)
        dst.append(d)
    if k_bins % 2 == 1 and sum(len(d) for d in dst) % 2 == 0:
        dst[-1] = dst[-1][:-1]
    rows = rng.randn(sum(SHAPE_FRAMES), k_bins) * np.exp(rng.randn(sum(SHAPE_FRAMES), 1))
    return src, dst, rows


def conversion_cases():
    """(name, source times, destination times) for two utterances (401 and 61 frames: the
    shorter one still ends beyond the 0.4 s anchor once stretched): uniform 5 ms -> 10 / 2.5 / 12.5 ms,
    and 5 ms stretched by scale_duration(1.7) and modify_duration([0.1, 0.2], [0, 0.05, 0.4, -1]) -> 5 ms."""
    from world._tables import frame_times
    from world.regrid import destination_times

    uniform = [frame_times(n, 5) for n in (401, 61)]
    out = [("5->%s" % p, uniform, [destination_times(t, p) for t in uniform]) for p in (10, 2.5, 12.5)]
    warped = []
    for t in uniform:
        t = t * 1.7
        warped.append(np.interp(t, np.r_[0, [0.1, 0.2], t[-1]], [0, 0.05, 0.4, t[-1]]))
    out.append(("stretched->5", warped, [destination_times(t, 5) for t in warped]))
    return out
