"""Polyphase resampling on the device — a drop-in for ``scipy.signal.resample_poly`` (the reference's callers resample
with it before the analysis: example/prosody.py:16-19), executed by the HIP kernel behind wh_resample_poly
(include/world_hip.h).  The filter is designed here with scipy's own recipe (firwin, the zero pads of resample_poly);
the device evaluates upfirdn's loop in scipy's summation order, so the result is scipy's, bit for bit."""
import functools
import math

import numpy as np

from . import _hip

MAX_RATE = 4096  # largest reduced up / down the library takes (wh_resample_poly)


def _output_len(len_h, n_in, up, down):
    """scipy.signal._upfirdn._output_len."""
    return ((n_in - 1) * up + len_h - 1) // down + 1


def _rates(up, down):
    for name, v in (("up", up), ("down", down)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer, float, np.floating)) or v != int(v):
            raise ValueError("resample_poly: %s must be an integer, got %r" % (name, v))
        if int(v) < 1:
            raise ValueError("resample_poly: %s must be >= 1, got %r" % (name, v))
    up, down = int(up), int(down)
    g = math.gcd(up, down)
    up, down = up // g, down // g
    if max(up, down) > MAX_RATE:
        raise ValueError("resample_poly: reduced ratio %d:%d beyond %d (the library's bound)" % (up, down, MAX_RATE))
    return up, down


def _window_key(window):
    return ("array", np.asarray(window, dtype=np.float64).tobytes()) if isinstance(window, (list, np.ndarray)) else window


@functools.lru_cache(maxsize=64)
def _base_filter(up, down, window_key):
    """(firwin(...) * up, half) as resample_poly builds them (float64; reduced up / down)."""
    from scipy.signal import firwin

    if isinstance(window_key, tuple) and len(window_key) == 2 and window_key[0] == "array":
        h = np.frombuffer(window_key[1], dtype=np.float64).copy()
        half = (h.size - 1) // 2
    else:
        max_rate = max(up, down)
        half = 10 * max_rate
        h = firwin(2 * half + 1, 1.0 / max_rate, window=window_key)
    h = h * up
    h.setflags(write=False)
    return h, half


def design(up, down, n_in, window=('kaiser', 5.0)):
    """The filter of resample_poly(x, up, down, window=window) for a signal of ``n_in`` samples, reduced ratio:
    dict(up, down, h (the padded FIR upfirdn runs), P (taps per phase), n_pre_remove, n_out).  The FIR is cached per
    (up, down, window, pads); what depends on the length is a few integer steps.  ``phases(d)``: scipy's phase table."""
    up, down = _rates(up, down)
    if isinstance(window, (list, np.ndarray)):
        w = np.asarray(window)
        if w.ndim > 1:
            raise ValueError("resample_poly: window must be 1-D")
        if np.iscomplexobj(w):
            raise ValueError("resample_poly: a complex FIR window is not supported")
    h0, half = _base_filter(up, down, _window_key(window))
    n_out = -(-n_in * up // down)
    n_pre_pad = down - half % down
    n_pre_remove = (half + n_pre_pad) // down
    n_post_pad = 0
    while _output_len(len(h0) + n_pre_pad + n_post_pad, n_in, up, down) < n_out + n_pre_remove:
        n_post_pad += 1
    h = _padded(up, down, _window_key(window), n_pre_pad, n_post_pad)
    P = -(-len(h) // up)
    return {"up": up, "down": down, "h": h, "P": P, "n_pre_remove": n_pre_remove, "n_out": n_out}


@functools.lru_cache(maxsize=64)
def _padded(up, down, window_key, n_pre_pad, n_post_pad):
    h0, _ = _base_filter(up, down, window_key)
    h = np.concatenate((np.zeros(n_pre_pad), h0, np.zeros(n_post_pad)))
    h.setflags(write=False)
    return h


def phases(d):
    """scipy's h_trans_flip of a design: h zero-padded to P*up, reshaped (P, up), transposed, each row reversed — [up][P]
    (the library builds the same table, tap-major, from ``h``)."""
    h, up, P = d["h"], d["up"], d["P"]
    hp = np.zeros(P * up)
    hp[:len(h)] = h
    return np.ascontiguousarray(hp.reshape(P, up).T[:, ::-1])


def _check_dtype(x):
    if np.iscomplexobj(x):
        raise TypeError("resample_poly: complex input is not supported (scipy computes it in complex arithmetic)")
    if np.issubdtype(x.dtype, np.floating) and x.dtype != np.float64:
        raise TypeError("resample_poly: %s input is not supported (scipy computes it in its own precision); pass float64"
                        % x.dtype)
    if not (x.dtype == np.float64 or np.issubdtype(x.dtype, np.integer) or x.dtype == np.bool_):
        raise TypeError("resample_poly: unsupported dtype %s" % x.dtype)


def resample_device(rt, x_d, in_off, ups, downs, window=('kaiser', 5.0), out=None):
    """Resample a resident ragged buffer: utterance u is x_d[in_off[u]:in_off[u+1]], resampled by ups[u] / downs[u].
    Enqueued on rt's stream; returns (y_d, out_off) with out_off a host int64 array.  ``out``: a contiguous float64
    device tensor of out_off[-1] elements to write instead of a new one."""
    in_off = np.ascontiguousarray(in_off, dtype=np.int64)
    n_utt = len(in_off) - 1
    if n_utt < 0 or np.any(np.diff(in_off) < 0) or (n_utt >= 0 and in_off[0] != 0):
        raise ValueError("resample: offsets must start at 0 and be monotone")
    ups = np.broadcast_to(np.asarray(ups), (n_utt,))
    downs = np.broadcast_to(np.asarray(downs), (n_utt,))
    up_r = np.empty(n_utt, dtype=np.int32)
    down_r = np.empty(n_utt, dtype=np.int32)
    filt_off = np.empty(n_utt, dtype=np.int64)
    filt_len = np.empty(n_utt, dtype=np.int64)
    pre = np.empty(n_utt, dtype=np.int64)
    n_out = np.empty(n_utt, dtype=np.int64)
    pieces, where, total = [], {}, 0
    designs = {}  # (up, down, n_in) -> design: a batch of equal lengths and rates designs once
    identity = np.ones(1)
    for u in range(n_utt):
        n_in = int(in_off[u + 1] - in_off[u])
        dk = (ups[u], downs[u], n_in)
        d = designs.get(dk)
        if d is None:
            up, down = _rates(ups[u], downs[u])
            if up == down == 1:
                # scipy returns a copy; the library runs the identity filter (one tap of 1.0: acc = 0.0 + x * 1.0 == x)
                d = {"up": 1, "down": 1, "h": identity, "n_pre_remove": 0, "n_out": n_in}
            else:
                d = design(up, down, n_in, window)
            designs[dk] = d
        key = id(d["h"])
        if key not in where:
            where[key] = total
            pieces.append(d["h"])
            total += len(d["h"])
        up_r[u], down_r[u] = d["up"], d["down"]
        filt_off[u], filt_len[u], pre[u], n_out[u] = where[key], len(d["h"]), d["n_pre_remove"], d["n_out"]
    out_off = np.concatenate([[0], np.cumsum(n_out)]).astype(np.int64)
    filters = np.ascontiguousarray(np.concatenate(pieces) if pieces else np.zeros(1), dtype=np.float64)
    if out is None:
        y_d = rt.empty((int(out_off[-1]),))
    elif out.dtype != rt.torch.float64 or not out.is_contiguous() or out.numel() != int(out_off[-1]):
        raise ValueError("resample: out must be a contiguous float64 tensor of %d elements" % int(out_off[-1]))
    else:
        y_d = out
    if n_utt and out_off[-1] > 0:
        _hip.check(rt.lib.wh_resample_poly(rt.ctx, rt.stream(), n_utt, _hip.i64p(in_off), _hip.i64p(out_off),
                                           _hip.i32p(up_r), _hip.i32p(down_r), _hip.i64p(filt_off), _hip.i64p(filt_len),
                                           _hip.i64p(pre), _hip.f64p(filters), len(filters), rt.ptr(x_d), rt.ptr(y_d)))
    return y_d, out_off


def rates_ratio(fs_in, fs_out):
    """(up, down) = (fs_out, fs_in) for integer rates, as prosody.py passes them (example/prosody.py:16-19)."""
    return _rates(fs_out, fs_in)


@_hip.serialised
def resample_poly(x, up, down, axis=0, window=('kaiser', 5.0), padtype='constant', cval=None):
    """scipy.signal.resample_poly(x, up, down, axis, window, padtype='constant', cval=None) on the device.  ``x``: 1-D, or
    2-D (a batch of the 1-D slices along ``axis``, one launch).  float64 or integer input (integers are converted to
    float64, as scipy does); float32 / complex input and other pad types raise instead of diverging from scipy."""
    x = np.asarray(x)
    if padtype != 'constant':
        raise ValueError("resample_poly: only padtype='constant' is supported, got %r" % (padtype,))
    if cval is not None and cval != 0:
        raise ValueError("resample_poly: only cval=None or 0 is supported, got %r" % (cval,))
    _check_dtype(x)
    if x.ndim not in (1, 2):
        raise ValueError("resample_poly: x must be 1-D or 2-D, got %d dimensions" % x.ndim)
    up_r, down_r = _rates(up, down)
    if up_r == down_r == 1:
        return x.copy()
    axis = axis % x.ndim
    moved = np.moveaxis(x, axis, -1)
    n_in = moved.shape[-1]
    rows = moved.astype(np.float64).reshape(int(np.prod(moved.shape[:-1])), n_in)
    n_out = -(-n_in * up_r // down_r)
    if rows.shape[0] == 0 or n_out == 0:
        out = np.zeros((rows.shape[0], n_out))
    else:
        rt = _hip.Runtime.get()
        with rt.on_stream():
            x_d = rt.to_device(rows.ravel())
            in_off = np.arange(rows.shape[0] + 1, dtype=np.int64) * n_in
            y_d, _ = resample_device(rt, x_d, in_off, up_r, down_r, window)
            out = rt.to_host(y_d).reshape(rows.shape[0], n_out)
    if x.ndim == 1:
        return out.reshape(n_out)
    shape = list(moved.shape[:-1]) + [n_out]
    return np.moveaxis(out.reshape(shape), -1, axis)
