"""The manifold vocoder's networks (World.encode_vae, world/main.py:367-384): stacks of Dense layers run on the
MI355X behind wh_dense_stack (include/world_hip.h), FP64 throughout, with the reference's glue around them fused into
the same launch — the `Xc -= mean` shift and get_context on the way in, the kept window of the decoder's output and
`Yc += mean` on the way out.

A ``DenseStack`` holds the layers' kernels, biases and activations.  It is built from ``(W, b, activation)`` triples, from
a Keras-like model (duck-typed: ``.layers`` with ``get_config()`` / ``get_weights()``; no Keras import), or from the
HDF5 file Keras 2 ``model.save`` writes, through the small read-only reader below (h5py is not needed).  No CPU
fallback: the *_device functions need the library and a GPU."""
import ctypes
import json

import numpy as np

from . import _hip

ACTIVATIONS = {"linear": 0, "relu": 1, "tanh": 2, "sigmoid": 3}
MAX_UNITS = 256      # widest layer the kernel's LDS tile holds (the last layer: its kept columns)
MAX_LAYERS = 16
MAX_INPUT = 2048     # widest first-layer input, after context stacking


class DenseStack:
    """Dense layers y = act(x W + b), W of shape (in, out) as Keras stores it.  The weights are kept as given
    (float32 for Keras models) and run on the device as exact float64 copies."""

    def __init__(self, layers):
        layers = list(layers)
        if not layers:
            raise ValueError("DenseStack: at least one layer is needed")
        if len(layers) > MAX_LAYERS:
            raise ValueError("DenseStack: %d layers exceed the limit of %d" % (len(layers), MAX_LAYERS))
        ws, bs, acts = [], [], []
        for i, layer in enumerate(layers):
            if len(layer) != 3:
                raise ValueError("DenseStack: layer %d must be a (W, b, activation) triple" % i)
            w, b, act = layer
            w = np.array(w, copy=True)
            b = np.array(b, copy=True)
            if w.dtype.kind != "f" or b.dtype.kind != "f":
                raise ValueError("DenseStack: layer %d: weights must be floating point" % i)
            if w.ndim != 2 or b.ndim != 1 or b.shape[0] != w.shape[1] or w.shape[0] < 1 or w.shape[1] < 1:
                raise ValueError("DenseStack: layer %d: W must be (in, out) and b (out,), got %s and %s"
                                 % (i, w.shape, b.shape))
            if i and w.shape[0] != ws[-1].shape[1]:
                raise ValueError("DenseStack: layer %d takes %d inputs but layer %d gives %d"
                                 % (i, w.shape[0], i - 1, ws[-1].shape[1]))
            if not (np.all(np.isfinite(w)) and np.all(np.isfinite(b))):
                raise ValueError("DenseStack: layer %d has non-finite weights" % i)
            if act is None:
                act = "linear"
            if act not in ACTIVATIONS:
                raise ValueError("DenseStack: layer %d: activation %r is not supported (linear, relu, tanh, sigmoid)"
                                 % (i, act))
            w.setflags(write=False)
            b.setflags(write=False)
            ws.append(w)
            bs.append(b)
            acts.append(act)
        self.weights, self.biases, self.activations = ws, bs, acts
        self.units = [w.shape[1] for w in ws]
        self.input_dim = ws[0].shape[0]
        # the host copy handed to wh_dense_stack (float64, layers one after the other) and its content tag
        self._w64 = np.concatenate([w.astype(np.float64).ravel() for w in ws])
        self._b64 = np.concatenate([b.astype(np.float64) for b in bs])
        self._units = np.array(self.units, dtype=np.int32)
        self._acts = np.array([ACTIVATIONS[a] for a in acts], dtype=np.int32)
        self.tag = _hip.table_tag(self._units, self._acts, self._w64, self._b64)

    def __len__(self):
        return len(self.weights)

    def __repr__(self):
        return "DenseStack(%d -> %s; %s)" % (self.input_dim, " -> ".join(map(str, self.units)),
                                             ", ".join(self.activations))

    def then(self, other):
        """This stack followed by ``other`` (encoder.then(decoder): one launch for both)."""
        return DenseStack(list(self.layers()) + list(other.layers()))

    def layers(self):
        return zip(self.weights, self.biases, self.activations)

    @classmethod
    def from_keras(cls, model):
        """From a Keras-like model: ``model.layers``, each with ``get_config()`` and ``get_weights()``.  InputLayer is
        skipped; any other layer that is not Dense is refused."""
        layers = []
        for layer in getattr(model, "layers"):
            kind = type(layer).__name__
            if kind == "InputLayer":
                continue
            if kind != "Dense":
                raise ValueError("DenseStack.from_keras: layer %r is a %s; only Dense layers are supported"
                                 % (getattr(layer, "name", "?"), kind))
            cfg = layer.get_config()
            wts = layer.get_weights()
            layers.append(_dense_triple(cfg, wts))
        return cls(layers)

    @classmethod
    def from_h5(cls, path):
        """From the HDF5 file of Keras 2 ``model.save`` (model_config and model_weights), read by H5File."""
        f = H5File(path)
        raw = f.attrs("/").get("model_config")
        if raw is None:
            raise ValueError("%s: no model_config attribute (not a Keras model file)" % path)
        config = json.loads(raw if isinstance(raw, str) else raw.decode("utf-8"))
        layers = []
        for spec in _config_layers(config):
            kind, lcfg = spec["class_name"], spec["config"]
            if kind == "InputLayer":
                continue
            if kind != "Dense":
                raise ValueError("DenseStack.from_h5: layer %r is a %s; only Dense layers are supported"
                                 % (lcfg.get("name"), kind))
            gpath = "/model_weights/" + lcfg["name"]
            names = f.attrs(gpath).get("weight_names", [])
            if isinstance(names, (str, bytes)):
                names = [names]
            wts = [f.dataset(gpath + "/" + (n.decode("utf-8") if isinstance(n, bytes) else n)) for n in names]
            layers.append(_dense_triple(lcfg, wts))
        return cls(layers)


def _config_layers(config):
    """The layer list of a Keras 2 model_config: Sequential (a list, or a dict with "layers") or a functional Model
    that is a single chain."""
    cfg = config.get("config", config)
    layers = cfg if isinstance(cfg, list) else cfg.get("layers")
    if not isinstance(layers, list):
        raise ValueError("model_config has no layer list")
    prev = None
    for spec in layers:
        nodes = spec.get("inbound_nodes")
        if nodes and prev is not None:
            srcs = [n[0] for node in nodes for n in node] if isinstance(nodes[0], list) else None
            if srcs is not None and srcs != [prev]:
                raise ValueError("model_config: layer %r does not follow %r: only a single chain of layers is supported"
                                 % (spec.get("name"), prev))
        prev = spec.get("name", spec.get("config", {}).get("name"))
    return layers


def _dense_triple(cfg, wts):
    act = cfg.get("activation", "linear")
    if act not in ACTIVATIONS:
        raise ValueError("Dense layer %r: activation %r is not supported (linear, relu, tanh, sigmoid)"
                         % (cfg.get("name"), act))
    use_bias = cfg.get("use_bias", True)
    if len(wts) != (2 if use_bias else 1):
        raise ValueError("Dense layer %r: expected %d weight arrays, got %d" % (cfg.get("name"), 2 if use_bias else 1,
                                                                                len(wts)))
    w = np.asarray(wts[0])
    b = np.asarray(wts[1]) if use_bias else np.zeros(w.shape[1] if w.ndim == 2 else 0, dtype=w.dtype)
    if w.ndim == 2 and "units" in cfg and cfg["units"] != w.shape[1]:
        raise ValueError("Dense layer %r: units %d but kernel %s" % (cfg.get("name"), cfg["units"], w.shape))
    return w, b, act


def as_stack(obj):
    """A DenseStack from a DenseStack, a Keras-like model or a path to a Keras HDF5 file."""
    if isinstance(obj, DenseStack):
        return obj
    if isinstance(obj, (str, bytes)) or hasattr(obj, "__fspath__"):
        return DenseStack.from_h5(obj)
    if hasattr(obj, "layers"):
        return DenseStack.from_keras(obj)
    raise TypeError("expected a DenseStack, a Keras-like model or a path to an HDF5 file, got %s" % type(obj).__name__)


# ---------------------------------------------------------------------------------------------------------------------
# A read-only HDF5 reader for what Keras 2's model.save writes with h5py's defaults: superblock version 0, version-1
# object headers with continuation blocks, symbol-table groups (version-1 B-tree, local heap, SNOD nodes), contiguous
# or compact little-endian float32 / float64 datasets, and fixed-length string attributes.  Anything else is refused
# with NotImplementedError naming what was met.
# ---------------------------------------------------------------------------------------------------------------------
_SIG = b"\x89HDF\r\n\x1a\n"


class H5File:
    def __init__(self, path):
        with open(path, "rb") as fh:
            self.buf = fh.read()
        self.path = path
        if self.buf[:8] != _SIG:
            raise ValueError("%s: not an HDF5 file (signature missing at offset 0)" % path)
        ver = self._u(8, 1)
        if ver != 0:
            raise NotImplementedError("%s: HDF5 superblock version %d (only version 0 is read)" % (path, ver))
        self.so, self.sl = self._u(13, 1), self._u(14, 1)
        if self.so not in (4, 8) or self.sl not in (4, 8):
            raise NotImplementedError("%s: HDF5 offset/length sizes %d/%d" % (path, self.so, self.sl))
        base = self._u(24, self.so)
        if base != 0:
            raise NotImplementedError("%s: HDF5 base address %d (only 0 is read)" % (path, base))
        root_entry = 24 + 4 * self.so
        self.root = self._u(root_entry + self.so, self.so)  # the root group's object header address

    # -- primitive reads, every one bounds-checked: a truncated file is refused, never read past its end --
    def _bytes(self, off, n):
        if off < 0 or n < 0 or off + n > len(self.buf):
            raise ValueError("%s: truncated or corrupt HDF5 file (read of %d bytes at %d, file has %d)"
                             % (self.path, n, off, len(self.buf)))
        return self.buf[off:off + n]

    def _u(self, off, n):
        return int.from_bytes(self._bytes(off, n), "little")

    def _undef(self, addr):
        return addr == (1 << (8 * self.so)) - 1

    # -- object headers --
    def _messages(self, addr):
        """(type, flags, data) of every message of the version-1 object header at addr, continuations followed."""
        if self._u(addr, 1) != 1:
            raise NotImplementedError("%s: object header version %d at %d (only version 1 is read)"
                                      % (self.path, self._u(addr, 1), addr))
        n_msgs = self._u(addr + 2, 2)
        size = self._u(addr + 8, 4)
        blocks = [(addr + 16, size)]  # the 12-byte prefix is padded to 16
        out = []
        seen = 0
        while blocks and seen < 100000:
            start, length = blocks.pop(0)
            p, end = start, start + length
            while p + 8 <= end and len(out) < n_msgs:
                mtype, msize, mflags = self._u(p, 2), self._u(p + 2, 2), self._u(p + 4, 1)
                data = self._bytes(p + 8, msize)
                p += 8 + msize
                seen += 1
                if mflags & 0x02:
                    raise NotImplementedError("%s: shared object header message (type %d)" % (self.path, mtype))
                if mtype == 0x10:  # continuation
                    blocks.append((int.from_bytes(data[:self.so], "little"),
                                   int.from_bytes(data[self.so:self.so + self.sl], "little")))
                out.append((mtype, mflags, data))
        return out

    def _dataspace(self, d):
        ver, rank, flags = d[0], d[1], d[2]
        if ver == 1:
            p = 8
        elif ver == 2:
            if d[3] == 2:  # null dataspace
                return None
            p = 4
        else:
            raise NotImplementedError("%s: dataspace message version %d" % (self.path, ver))
        dims = tuple(int.from_bytes(d[p + i * self.sl:p + (i + 1) * self.sl], "little") for i in range(rank))
        return dims

    def _datatype(self, d):
        cls, ver = d[0] & 0x0F, d[0] >> 4
        bits = d[1] | (d[2] << 8) | (d[3] << 16)
        size = int.from_bytes(d[4:8], "little")
        if cls == 1:  # floating point
            if bits & 0x41 != 0:
                raise NotImplementedError("%s: big-endian or VAX floating point data" % self.path)
            if size not in (4, 8):
                raise NotImplementedError("%s: %d-byte floating point data" % (self.path, size))
            return ("<f%d" % size, size)
        if cls == 3:  # fixed-length string
            return ("S", size)
        if cls == 0:  # fixed-point integer
            if bits & 0x01:
                raise NotImplementedError("%s: big-endian integer data" % self.path)
            return (("<i%d" if bits & 0x08 else "<u%d") % size, size)
        if cls == 9:
            if bits & 0x0F != 1:
                raise NotImplementedError("%s: variable-length sequence data" % self.path)
            return ("V", size)  # a variable-length string: (length, global heap collection, object index)
        raise NotImplementedError("%s: datatype class %d (version %d)" % (self.path, cls, ver))

    def _decode(self, raw, dtype, size, dims):
        count = int(np.prod(dims)) if dims else 1
        if len(raw) < count * size:
            raise ValueError("%s: truncated or corrupt HDF5 data" % self.path)
        if dtype in ("S", "V"):
            vals = [raw[i * size:(i + 1) * size] for i in range(count)]
            if dtype == "V":
                vals = [self._global_object(int.from_bytes(v[4:4 + self.so], "little"),
                                            int.from_bytes(v[4 + self.so:8 + self.so], "little"))[:int.from_bytes(v[:4], "little")]
                        for v in vals]
            vals = [v.split(b"\x00", 1)[0] for v in vals]
            return vals[0] if not dims else vals
        a = np.frombuffer(raw, dtype=dtype, count=count)
        return a.reshape(dims) if dims else a[0]

    def _attributes(self, addr):
        out = {}
        for mtype, _, d in self._messages(addr):
            if mtype == 0x15:
                raise NotImplementedError("%s: dense attribute storage (attribute info message)" % self.path)
            if mtype != 0x0C:
                continue
            ver = d[0]
            if ver == 1:
                nlen, tlen, slen = (int.from_bytes(d[i:i + 2], "little") for i in (2, 4, 6))
                pad = lambda n: (n + 7) & ~7  # noqa: E731
                p = 8
                name = d[p:p + nlen].split(b"\x00", 1)[0].decode("utf-8")
                p += pad(nlen)
                dt = d[p:p + tlen]
                p += pad(tlen)
                ds = d[p:p + slen]
                p += pad(slen)
            elif ver in (2, 3):
                if d[1] & 0x03:
                    raise NotImplementedError("%s: attribute with a shared datatype or dataspace" % self.path)
                nlen, tlen, slen = (int.from_bytes(d[i:i + 2], "little") for i in (2, 4, 6))
                p = 8 + (1 if ver == 3 else 0)
                name = d[p:p + nlen].split(b"\x00", 1)[0].decode("utf-8")
                p += nlen
                dt = d[p:p + tlen]
                p += tlen
                ds = d[p:p + slen]
                p += slen
            else:
                raise NotImplementedError("%s: attribute message version %d" % (self.path, ver))
            dtype, size = self._datatype(dt)
            dims = self._dataspace(ds)
            out[name] = self._decode(d[p:], dtype, size, dims or ())
        return out

    def _global_object(self, coll, index):
        """Object `index` of the global heap collection at coll (variable-length strings live there)."""
        if self._bytes(coll, 4) != b"GCOL":
            raise ValueError("%s: corrupt global heap collection at %d" % (self.path, coll))
        end = coll + self._u(coll + 8, self.sl)
        p = coll + 8 + self.sl
        while p + 8 + self.sl <= end:
            idx, size = self._u(p, 2), self._u(p + 8, self.sl)
            if idx == 0:
                break
            if idx == index:
                return self._bytes(p + 8 + self.sl, size)
            p += 8 + self.sl + ((size + 7) & ~7)
        raise ValueError("%s: global heap object %d missing from the collection at %d" % (self.path, index, coll))

    # -- groups --
    def _heap_name(self, heap, off):
        if self._bytes(heap, 4) != b"HEAP":
            raise ValueError("%s: corrupt local heap at %d" % (self.path, heap))
        data = self._u(heap + 8 + 2 * self.sl, self.so)
        p = data + off
        end = self.buf.find(b"\x00", p)
        if end < 0:
            raise ValueError("%s: truncated or corrupt HDF5 file (unterminated name)" % self.path)
        return self.buf[p:end].decode("utf-8")

    def _btree_children(self, node, heap, out, depth=0):
        if depth > 64 or self._bytes(node, 4) != b"TREE":
            raise ValueError("%s: corrupt group B-tree at %d" % (self.path, node))
        ntype, level, used = self._u(node + 4, 1), self._u(node + 5, 1), self._u(node + 6, 2)
        if ntype != 0:
            raise NotImplementedError("%s: B-tree of node type %d in a group" % (self.path, ntype))
        p = node + 8 + 2 * self.so  # key 0, child 0, key 1, ...
        for _ in range(used):
            child = self._u(p + self.sl, self.so)
            p += self.sl + self.so
            if level > 0:
                self._btree_children(child, heap, out, depth + 1)
            else:
                if self._bytes(child, 4) != b"SNOD":
                    raise ValueError("%s: corrupt symbol table node at %d" % (self.path, child))
                n = self._u(child + 6, 2)
                e = child + 8
                for _ in range(n):
                    out[self._heap_name(heap, self._u(e, self.so))] = self._u(e + self.so, self.so)
                    e += 2 * self.so + 24
        return out

    def _children(self, addr):
        for mtype, _, d in self._messages(addr):
            if mtype == 0x11:
                btree = int.from_bytes(d[:self.so], "little")
                heap = int.from_bytes(d[self.so:2 * self.so], "little")
                return self._btree_children(btree, heap, {})
            if mtype in (0x02, 0x06, 0x0A):
                raise NotImplementedError("%s: new-style (link message) group" % self.path)
        return {}

    def _lookup(self, path):
        addr = self.root
        for part in [p for p in path.split("/") if p]:
            kids = self._children(addr)
            if part not in kids:
                raise KeyError("%s: no object %r in %s" % (self.path, part, path))
            addr = kids[part]
        return addr

    # -- public --
    def attrs(self, path):
        """The attributes of the group or dataset at path, strings as bytes."""
        return self._attributes(self._lookup(path))

    def keys(self, path="/"):
        return sorted(self._children(self._lookup(path)))

    def dataset(self, path):
        """The dataset at path as a NumPy array (its stored dtype)."""
        addr = self._lookup(path)
        dims = dtype = layout = None
        for mtype, _, d in self._messages(addr):
            if mtype == 0x01:
                dims = self._dataspace(d)
            elif mtype == 0x03:
                dtype = self._datatype(d)
            elif mtype == 0x08:
                layout = d
            elif mtype == 0x0B:
                raise NotImplementedError("%s: %s: filter pipeline (compressed or filtered data)" % (self.path, path))
        if dims is None or dtype is None or layout is None:
            raise ValueError("%s: %s is not a dataset" % (self.path, path))
        ver = layout[0]
        if ver != 3:
            raise NotImplementedError("%s: %s: data layout message version %d" % (self.path, path, ver))
        cls = layout[1]
        size = dtype[1] * (int(np.prod(dims)) if dims else 1)
        if cls == 0:  # compact
            n = int.from_bytes(layout[2:4], "little")
            raw = layout[4:4 + n]
        elif cls == 1:  # contiguous
            a = int.from_bytes(layout[2:2 + self.so], "little")
            if self._undef(a):
                raise ValueError("%s: %s has no data written" % (self.path, path))
            raw = self._bytes(a, size)
        elif cls == 2:
            raise NotImplementedError("%s: %s: chunked data layout" % (self.path, path))
        else:
            raise NotImplementedError("%s: %s: data layout class %d" % (self.path, path, cls))
        if dtype[0] in ("S", "V"):
            raise NotImplementedError("%s: %s: string dataset" % (self.path, path))
        return np.array(self._decode(raw, dtype[0], dtype[1], dims))


# ---------------------------------------------------------------------------------------------------------------------
# Device
# ---------------------------------------------------------------------------------------------------------------------
def dense_stack_device(rt, x_d, stack, seg_off=None, window=0, in_shift=None, out_cols=None, out_shift=None,
                       tap_layer=-1, tap_f32=False):
    """Run ``stack`` over the rows of the frame-major device tensor x_d (n_rows, d) in one launch.

    The first layer sees row i with its context, rows i-window .. i+window side by side (get_context, main.py:360-365),
    clamped to the row's own segment of ``seg_off`` (n_seg + 1 row offsets; default: one segment), each row minus
    ``in_shift`` (d values).  The last layer keeps its columns ``out_cols = (c0, n)`` (default: all), plus ``out_shift``
    (n values).  Returns ``out`` (n_rows, n), or ``(tap, out)`` when ``tap_layer`` >= 0 also writes that layer's output
    (rounded to float32 when ``tap_f32``, for the next layer as well).  Every row's result is independent of the other
    rows."""
    stack = as_stack(stack)
    n, d = (int(v) for v in x_d.shape)
    window = int(window)
    if window < 0:
        raise ValueError("dense_stack: window must be >= 0")
    if (2 * window + 1) * d != stack.input_dim:
        raise ValueError("dense_stack: the stack takes %d inputs, rows of %d with window %d give %d"
                         % (stack.input_dim, d, window, (2 * window + 1) * d))
    if stack.input_dim > MAX_INPUT:
        raise ValueError("dense_stack: input width %d exceeds the limit of %d" % (stack.input_dim, MAX_INPUT))
    for i, u in enumerate(stack.units[:-1]):
        if u > MAX_UNITS:
            raise ValueError("dense_stack: layer %d has %d units, the limit is %d" % (i, u, MAX_UNITS))
    c0, n_out = (0, stack.units[-1]) if out_cols is None else (int(out_cols[0]), int(out_cols[1]))
    if c0 < 0 or n_out < 1 or c0 + n_out > stack.units[-1]:
        raise ValueError("dense_stack: kept columns [%d, %d) outside the last layer's %d" % (c0, c0 + n_out,
                                                                                            stack.units[-1]))
    if n_out > MAX_UNITS:
        raise ValueError("dense_stack: %d kept output columns exceed the limit of %d" % (n_out, MAX_UNITS))
    tap_layer = int(tap_layer)
    if tap_layer >= len(stack) - 1:
        raise ValueError("dense_stack: tap_layer must name a layer before the last")
    seg = np.array([0, n] if seg_off is None else seg_off, dtype=np.int64)
    if seg.ndim != 1 or len(seg) < 2 or seg[0] != 0 or seg[-1] != n or np.any(np.diff(seg) < 0):
        raise ValueError("dense_stack: seg_off must run from 0 to %d without decreasing" % n)
    vp = ctypes.c_void_p

    def host_vec(v, k, what):
        if v is None:
            return None, vp(None)
        a = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
        if a.shape[0] != k:
            raise ValueError("dense_stack: %s must have %d values, got %d" % (what, k, a.shape[0]))
        return a, a.ctypes.data_as(vp)

    ish, ish_p = host_vec(in_shift, d, "in_shift")
    osh, osh_p = host_vec(out_shift, n_out, "out_shift")
    out = rt.empty((n, n_out))
    tap = rt.empty((n, stack.units[tap_layer])) if tap_layer >= 0 else None
    if x_d.stride(1) != 1:
        raise ValueError("dense_stack: rows must be contiguous")
    _hip.check(rt.lib.wh_dense_stack(
        rt.ctx, rt.stream(), rt.ptr(x_d), n, d, int(x_d.stride(0)) if n else d,
        _hip.i64p(seg), len(seg) - 1, window, ish_p, len(stack),
        stack._units.ctypes.data_as(vp), stack._acts.ctypes.data_as(vp), stack._w64.ctypes.data_as(vp),
        stack._b64.ctypes.data_as(vp), c0, n_out, tap_layer, rt.ptr(tap) if tap is not None else vp(None),
        stack.units[tap_layer] if tap_layer >= 0 else 0, int(bool(tap_f32)), osh_p, rt.ptr(out), n_out, stack.tag))
    return (tap, out) if tap_layer >= 0 else out


def vae_device(rt, x_d, encoder, decoder, window=0, mean=None, seg_off=None):
    """The networks of encode_vae (main.py:369-379) in one launch: the encoder and decoder as one stack with the latent
    as the tap.  x_d: (N, n0-1) device MCEP without the energy column.  Returns (Z_d, Y_d): the latent and the decoded
    MCEP, columns window*(n0-1) .. (window+1)*(n0-1) of the decoder's output, plus ``mean``.  The latent is rounded to
    float32 on its way to the decoder, as Keras' ``decoder.predict(encoder.predict(x))`` hands it on, so that
    decoding the returned latent alone (decode_vae_device) gives the same bits."""
    enc, dec = as_stack(encoder), as_stack(decoder)
    d = int(x_d.shape[1])
    if dec.input_dim != enc.units[-1]:
        raise ValueError("vae: the decoder takes %d inputs, the encoder gives %d" % (dec.input_dim, enc.units[-1]))
    if dec.units[-1] < (window + 1) * d:
        raise ValueError("vae: the decoder gives %d columns, window %d keeps %d .. %d"
                         % (dec.units[-1], window, window * d, (window + 1) * d))
    both = _joined(enc, dec)
    return dense_stack_device(rt, x_d, both, seg_off=seg_off, window=window, in_shift=mean, out_cols=(window * d, d),
                              out_shift=mean, tap_layer=len(enc) - 1, tap_f32=True)


def decode_vae_device(rt, z_d, decoder, d, window=0, mean=None, seg_off=None):
    """The decoder half of vae_device on a (possibly edited) latent z_d (N, latent): columns window*d .. (window+1)*d
    of its output plus ``mean``."""
    dec = as_stack(decoder)
    if dec.units[-1] < (window + 1) * d:
        raise ValueError("vae: the decoder gives %d columns, window %d keeps %d .. %d"
                         % (dec.units[-1], window, window * d, (window + 1) * d))
    return dense_stack_device(rt, z_d, dec, seg_off=seg_off, out_cols=(window * d, d), out_shift=mean)


_JOINED = {}


def _joined(enc, dec):
    """encoder.then(decoder), kept per pair of stacks (its content tag is computed once)."""
    key = (enc.tag, dec.tag)
    st = _JOINED.get(key)
    if st is None:
        if len(_JOINED) > 16:
            _JOINED.clear()
        st = _JOINED[key] = enc.then(dec)
    return st
