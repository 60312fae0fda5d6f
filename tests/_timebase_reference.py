"""The synthesis time base in plain NumPy, field by field — the reference of tests/test_hip_timebase.py.

Restates world/synthesis.py:118-152 (time_base_generation, get_spectral_parameters' frame pair and weight) and
:49-51, 65, 69 (temporal_position_index, noise_size, the per-pulse voicing) of the reference, on top of
oracle.resynth.pulse_train and with the very lines of oracle.resynth.synthesis_np that derive the per-pulse quantities.
Everything is an integer or the result of IEEE-exact operations in the reference's order, so the device is compared
with it by equality of bits (tests/test_timebase_reference_host.py pins this module against synthesis_np's aux
outputs)."""
from decimal import ROUND_HALF_UP, Decimal

import numpy as np

from oracle import common as C
from oracle import resynth


class NoPulse(Exception):
    """the reference asserts (world/synthesis.py:131)"""


def final_f0(f0, vuv, limit):
    """The F0 stage's raw output as World.encode leaves it after CheapTrick (voiced below 3 fs / (fft_size - 3) ->
    500 Hz, world/cheaptrick.py:26-27,32-33) and D4C (unvoiced -> 0, world/d4c.py:32): what the fused form of the time
    base (f0_low_limit > 0) reads through prep_kernel's final_f0."""
    f0 = np.asarray(f0, dtype=np.float64)
    vuv = np.asarray(vuv, dtype=np.float64)
    return np.where(vuv == 0.0, 0.0, np.where(f0 < limit, 500.0, f0))


def low_limit(fs, fft_size):
    return 3.0 * fs / (fft_size - 3.0)


def timebase_np(tp, f0, vuv, fs, default_f0=500):
    """Every field wh_synthesis_timebase_read returns for one utterance, plus what the case table's conditions need:
    ``at`` (0-based sample in front of each phase wrap), ``ny``, ``same`` (t1 == t2), ``draws`` (sum max(3, noise_size))
    and ``pos_idx``.  Raises NoPulse where the reference asserts, IndexError where it indexes outside the wrapped
    phase."""
    tp = np.asarray(tp, dtype=np.float64)
    f0 = np.asarray(f0, dtype=np.float64)
    vuv = np.asarray(vuv, dtype=np.float64)
    # synthesis.py:39, 121-129
    t = np.arange(tp[0], tp[-1] + 1 / fs, 1 / fs)
    f0_i = C.lerp_extrap(tp, f0, t)
    vuv_i = C.lerp_extrap(tp, vuv, t) > 0.5
    f0_i = f0_i * vuv_i
    f0_i[f0_i == 0] = f0_i[f0_i == 0] + default_f0
    total = np.cumsum(2 * np.pi * f0_i / fs)
    wrap = np.remainder(total, 2 * np.pi)
    at = np.nonzero(np.abs(np.diff(wrap)) > np.pi)[0]
    if len(at) == 0:
        raise NoPulse()
    times = t[:-1][at]
    idx = np.array([int(Decimal(e * fs).quantize(0, ROUND_HALF_UP)) for e in times], dtype=np.int64) + 1
    ny = len(t)
    if idx.min() < 1 or idx.max() > ny - 1:  # (NumPy would wrap a negative index silently)
        raise IndexError("pulse index outside 1 .. ny - 1")
    # synthesis.py:134-138
    y1 = wrap[idx - 1] - 2.0 * np.pi
    y2 = wrap[idx]
    shift = (-y1 / (y2 - y1)) / fs
    # the same through the oracle's own function: one source of truth for the four fields it returns
    o_times, o_idx, o_shift, o_vuv_i, o_t = resynth.pulse_train(tp, f0, fs, vuv, default_f0)
    assert np.array_equal(o_times, times) and np.array_equal(o_idx, idx) and np.array_equal(o_vuv_i, vuv_i)
    assert np.array_equal(o_shift.view(np.int64), shift.view(np.int64)) and np.array_equal(o_t, t)
    # synthesis.py:50-52, 144-159 (oracle.resynth.synthesis_np's lines)
    pos_idx = C.lerp_extrap(tp, np.arange(1, len(tp) + 1, dtype=np.float64), times)
    pos_idx = np.maximum(1, np.minimum(len(tp), pos_idx))
    lo = np.floor(pos_idx).astype(np.int64) - 1
    hi = np.ceil(pos_idx).astype(np.int64) - 1
    t1 = tp[lo]
    t2 = tp[hi]
    xq = np.maximum(t1, np.minimum(t2, times))
    same = t1 == t2
    with np.errstate(invalid="ignore", divide="ignore"):
        b = np.where(same, 0.0, (xq - t1) / (t2 - t1))
    assert np.all((0 <= b) & (b <= 1))  # synthesis.py:160
    # synthesis.py:66, 93, 69
    nxt = idx[np.minimum(len(idx) - 1, np.arange(len(idx)) + 1)]
    noise_size = nxt - idx
    draws = np.maximum(3, noise_size)
    off = np.concatenate([[0], np.cumsum(draws)])
    return {
        "count": len(idx), "pidx": idx, "time": times, "shift": shift, "noff": off[:-1].astype(np.int64),
        "noise_size": noise_size.astype(np.int32), "vuv": (vuv_i[idx - 1] >= 0.5).astype(np.int32),
        "row_lo": lo, "row_hi": hi, "weight": np.where(same, -1.0, b), "phase": total, "vuv_s": vuv_i.astype(np.uint8),
        "at": at, "ny": ny, "same": same, "draws": int(draws.sum()), "pos_idx": pos_idx, "b": b, "t": t, "wrap": wrap,
    }


INT_FIELDS = ("pidx", "noff", "noise_size", "vuv", "row_lo", "row_hi", "vuv_s")
BIT_FIELDS = ("time", "shift", "weight", "phase")


def mismatches(got, want, n=None):
    """Names of the fields in which a read-back ``got`` differs from the reference ``want`` (its first ``n`` pulses;
    all of them by default): integers as integers, doubles as int64 views.  Empty: equal."""
    bad = []
    n = want["count"] if n is None else n
    if got["count"] != n:
        bad.append("count %d != %d" % (got["count"], n))
        return bad
    for k in INT_FIELDS + BIT_FIELDS:
        per_sample = k in ("phase", "vuv_s")
        g = np.asarray(got[k])
        w = np.asarray(want[k]) if per_sample else np.asarray(want[k])[:n]
        if g.shape != w.shape:
            bad.append("%s shape %s != %s" % (k, g.shape, w.shape))
        elif k in BIT_FIELDS:
            ne = np.nonzero(np.ascontiguousarray(g, dtype=np.float64).view(np.int64) !=
                            np.ascontiguousarray(w, dtype=np.float64).view(np.int64))[0]
            if len(ne):
                bad.append("%s at %d: %r != %r (%d differ)" % (k, ne[0], g[ne[0]], w[ne[0]], len(ne)))
        else:
            ne = np.nonzero(g.astype(np.int64) != w.astype(np.int64))[0]
            if len(ne):
                bad.append("%s at %d: %d != %d (%d differ)" % (k, ne[0], g[ne[0]], w[ne[0]], len(ne)))
    return bad
