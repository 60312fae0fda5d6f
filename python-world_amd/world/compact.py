"""Compact encodings: what a corpus builder stores instead of the dense analysis tensors — f0, vuv, an n0-coefficient
mel-cepstrum (the reference's encode_mcep, world/main.py:324-341, as test/spectralFeatures.py:31-33 computes it) and D4C's
band aperiodicity ('coarse_ap', world/d4c.py:57,62) — produced on the device, stored, reloaded and expanded again on the
device just before the synthesis, without a dense tensor crossing PCIe.

    enc = wb.encode(xs, 16000, want_coarse=True)        # BatchEncoding, resident
    ce = enc.compact(n0=40)                              # CompactEncoding, resident: 360 B per frame instead of 8 232
    ce.to_host().save_npz("batch0.npz")                  # one pinned block over PCIe, one file per batch
    ...
    ce = CompactEncoding.load_npz("batch0.npz").to_device(wb.rt)
    y, y_off = wb.decode_device(ce.expand(wb))           # imcep_device + wh_aperiodicity_from_bands, then the usual decode

The expansion of the spectrum is decode_mcep (world/main.py:343-358), which hard-codes 16 kHz and the 0-8000 Hz warp:
`compact(n0=...)` therefore refuses other rates; `compact(n0=None)` keeps the dense spectrogram and codes the aperiodicity
only, at every rate; `compact(lsf_order=p)` codes the spectrum as line spectral frequencies (world/lsf.py: rows
[log E, w_1 .. w_p], expanded by ilsf_device), at every rate.  Requiem encodings already hold the band form
(world/d4cRequiem.py:27-40): it is carried as it is.

save_npz / load_npz and the argument checks are host code and need neither the library nor a GPU."""
import numpy as np

# tensors of a compact encoding in the order they travel in (all float64, frame-major)
_FIELDS = ("temporal_positions", "f0", "vuv", "mcep", "lsf", "spectrogram", "band_ap", "ap_gate")


def d4c_band_layout(fs, is_requiem=False):
    """(frequency_interval, number of bands) of d4c() / d4cRequiem() at ``fs`` (world/d4c.py:25-27,34; d4cRequiem.py:19)."""
    interval = 2000 if (fs < 16000 and not is_requiem) else 3000
    return interval, int(np.floor(np.min([15000, fs / 2 - interval]) / interval))


def check_compact_args(fs, fft_size, n0, where="compact"):
    """Raises ValueError for what the spectral side cannot code; touches no device."""
    if n0 is None:
        return
    if fs != 16000:
        raise ValueError("%s: the mel-cepstrum is expanded by decode_mcep, which hard-codes fs = 16000 Hz and the 0-8000 Hz "
                         "warp (world/main.py:347-355): fs = %r cannot be rebuilt; compact(n0=None) keeps the dense "
                         "spectrogram and codes the aperiodicity only" % (where, fs))
    if int(n0) != n0 or n0 < 2 or n0 > fft_size // 2 + 1:
        raise ValueError("%s: n0 must be an integer in [2, fft_size // 2 + 1 = %d], got %r" % (where, fft_size // 2 + 1, n0))


class CompactEncoding:
    """A batch of utterances as f0 / vuv / frame times [F], mel-cepstrum [F][n0] (or, ``n0 is None``, the dense spectrogram
    [F][K], or line spectral frequencies ``lsf`` [F][lsf_order + 1]; ``kind`` says which), band aperiodicity [F][nap] with
    D4C's voicing gate [F] (Requiem: the dB rows [F][nap + 2], no gate) — frames of all utterances one after the other,
    utterance u being rows frame_off[u]:frame_off[u+1].  The tensors are torch device tensors (``rt`` is the runtime they
    live on) or, after to_host() / load_npz(), NumPy arrays (``rt is None``)."""

    def __init__(self, rt, fs, fft_size, frame_period, is_requiem, n0, lowhz, highhz, frame_off, temporal_positions, f0,
                 vuv, mcep, band_ap, ap_gate, spectrogram=None, tp_host=None, mcep_fs=None, lsf=None, lsf_order=None):
        self.rt, self.fs, self.fft_size, self.frame_period = rt, fs, int(fft_size), frame_period
        self.is_requiem, self.n0, self.lowhz, self.highhz = bool(is_requiem), n0, lowhz, highhz
        self.frame_off = np.ascontiguousarray(frame_off, dtype=np.int64)
        self.temporal_positions, self.f0, self.vuv = temporal_positions, f0, vuv
        self.mcep, self.spectrogram, self.band_ap, self.ap_gate = mcep, spectrogram, band_ap, ap_gate
        # the third spectral kind: line spectral frequencies, rows [log E, w_1 .. w_p] (world/lsf.py), at any rate
        self.lsf = lsf
        self.lsf_order = None if lsf is None else (int(np.shape(lsf)[1]) - 1 if lsf_order is None else int(lsf_order))
        self.tp_host = tp_host
        # the rate encode_mcep was told (its `fs` argument): the encoding's own unless compact(mcep_fs=...) said otherwise
        self.mcep_fs = None if mcep is None else (fs if mcep_fs is None else mcep_fs)
        self._check_shapes()

    # ---- checks (host) --------------------------------------------------------------------------------------------
    def _check_shapes(self):
        fo = self.frame_off
        if fo.ndim != 1 or len(fo) < 1 or fo[0] != 0 or np.any(np.diff(fo) < 0):
            raise ValueError("CompactEncoding: frame_off must start at 0 and not decrease")
        nf = int(fo[-1])
        for name in ("temporal_positions", "f0", "vuv") + (() if self.is_requiem else ("ap_gate",)):
            shape = tuple(getattr(self, name).shape)
            if shape != (nf,):
                raise ValueError("CompactEncoding: '%s' must hold one value per frame (%d), got shape %s" % (name, nf, shape))
        if self.lsf is not None:
            from .lsf import check_order
            if self.mcep is not None or self.spectrogram is not None:
                raise ValueError("CompactEncoding: exactly one of mcep, lsf and spectrogram is kept")
            check_order(self.lsf_order, "CompactEncoding", self.fft_size // 2 + 1)
            want = ("lsf", (nf, self.lsf_order + 1))
        elif (self.mcep is None) == (self.spectrogram is None):
            raise ValueError("CompactEncoding: exactly one of mcep and spectrogram is kept")
        elif self.mcep is not None:
            check_compact_args(self.mcep_fs, self.fft_size, self.n0, "CompactEncoding")
            want = ("mcep", (nf, int(self.n0)))
        else:
            want = ("spectrogram", (nf, self.fft_size // 2 + 1))
        if tuple(getattr(self, want[0]).shape) != want[1]:
            raise ValueError("CompactEncoding: '%s' must be %s, got %s" % (want[0], want[1], tuple(getattr(self, want[0]).shape)))
        _, nap = d4c_band_layout(self.fs, self.is_requiem)
        bands = nap + 2 if self.is_requiem else nap
        if nap < 1 or tuple(self.band_ap.shape) != (nf, bands):
            raise ValueError("CompactEncoding: 'band_ap' must be (%d, %d) at fs = %r, got %s"
                             % (nf, bands, self.fs, tuple(self.band_ap.shape)))

    @property
    def kind(self):
        """How the spectrum is kept: 'mcep', 'lsf' or 'spectrogram'."""
        return "lsf" if self.lsf is not None else ("mcep" if self.mcep is not None else "spectrogram")

    @property
    def n_utt(self):
        return len(self.frame_off) - 1

    @property
    def total_frames(self):
        return int(self.frame_off[-1])

    def _tensors(self):
        return [(k, getattr(self, k)) for k in _FIELDS if getattr(self, k) is not None]

    def nbytes(self):
        """Bytes of the per-frame tensors: what to_host() / to_device() move."""
        return int(sum(int(np.prod(t.shape)) for _, t in self._tensors())) * 8

    def _like(self, rt, arrays, tp_host):
        return CompactEncoding(rt, self.fs, self.fft_size, self.frame_period, self.is_requiem, self.n0, self.lowhz,
                               self.highhz, self.frame_off, arrays["temporal_positions"], arrays["f0"], arrays["vuv"],
                               arrays.get("mcep"), arrays["band_ap"], arrays.get("ap_gate"), arrays.get("spectrogram"),
                               tp_host=tp_host, mcep_fs=self.mcep_fs, lsf=arrays.get("lsf"), lsf_order=self.lsf_order)

    # ---- PCIe: one pinned block per direction ----------------------------------------------------------------------
    def to_host(self):
        """The same encoding with NumPy arrays: the tensors leave as ONE block through pinned host memory
        (Runtime.to_host); only the compact tensors cross PCIe."""
        if self.rt is None:
            return self
        rt = self.rt
        parts = self._tensors()
        with rt.lock, rt.on_stream():
            flat = rt.to_host(rt.torch.cat([t.reshape(-1) for _, t in parts]))
        arrays, at = {}, 0
        for k, t in parts:
            n = int(np.prod(t.shape))
            arrays[k] = flat[at:at + n].reshape(tuple(t.shape))
            at += n
        return self._like(None, arrays, arrays["temporal_positions"])

    def to_device(self, rt):
        """The same encoding resident on ``rt``'s device: one upload through a pinned staging block."""
        if self.rt is not None:
            if self.rt.index != rt.index:
                return self.to_host().to_device(rt)
            return self
        parts = self._tensors()
        with rt.lock, rt.on_stream():
            flat = rt.to_device_concat([np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for _, a in parts])
        arrays, at = {}, 0
        for k, a in parts:
            n = int(np.prod(a.shape))
            arrays[k] = flat[at:at + n].view(tuple(a.shape))
            at += n
        return self._like(rt, arrays, np.array(self.temporal_positions, dtype=np.float64))

    @classmethod
    def from_host(cls, host, rt):
        """``host.to_device(rt)`` for an encoding that to_host() / load_npz() / from_dicts() made."""
        return host.to_device(rt)

    # ---- expansion ---------------------------------------------------------------------------------------------------
    def expand(self, world_batch):
        """BatchEncoding on ``world_batch``'s device, ready for decode_device: spectrogram = imcep_device(mcep, fft_size)
        (decode_mcep), aperiodicity = wh_aperiodicity_from_bands(band_ap, ap_gate) — D4C's own rows, bit for bit;
        f0 / vuv / frame times are passed through, and so are a Requiem encoding's band rows."""
        from .batch import BatchEncoding
        from .d4c import aperiodicity_from_bands_device
        from .features import imcep_device

        rt = world_batch.rt
        ce = self.to_device(rt)
        with rt.lock, rt.on_stream():
            batch = rt.make_batch(np.zeros(ce.n_utt + 1, dtype=np.int64), ce.frame_off)
            if ce.lsf is not None:
                from .lsf import ilsf_device
                spec = ilsf_device(rt, ce.lsf, ce.fft_size)
            else:
                spec = ce.spectrogram if ce.mcep is None else imcep_device(rt, ce.mcep, ce.fft_size)
            if ce.is_requiem:
                ap = ce.band_ap
            else:
                ap = aperiodicity_from_bands_device(rt, ce.band_ap, ce.ap_gate, ce.fs, ce.fft_size)
        return BatchEncoding(rt, batch, ce.fs, ce.temporal_positions, ce.f0, ce.vuv, spec, ap, ce.fft_size, ce.is_requiem,
                             ce.frame_period, tp_host=None if ce.tp_host is None else np.array(ce.tp_host))

    # ---- dynamic features and parameter generation (world/dynamics.py) ---------------------------------------------------
    def dynamic_features(self, windows=None):
        """What a statistical model of this encoding is trained on: {"mcep": [F][n_win n0], "band_ap": [F][n_win bands]}
        ({"lsf": [F][n_win (p + 1)], "band_ap": ...} for line spectral frequencies),
        column w * d + c being window w (static, delta, delta-delta for the default HTS_WINDOWS) over column c; no window
        reaches across an utterance.  Device tensors; the encoding must be resident."""
        from .dynamics import HTS_WINDOWS, compact_dynamic_features
        return compact_dynamic_features(self, HTS_WINDOWS if windows is None else windows)

    def with_trajectories(self, mcep=None, band_ap=None, windows=None, lsf=None, min_gap=None):
        """A new CompactEncoding whose 'mcep' / 'band_ap' are the maximum-likelihood tracks (world.dynamics.mlpg_device) of
        the given (mean, var) pairs — mean [F][n_win d] laid out like dynamic_features(), var the same shape or one row
        [n_win d]; None keeps this encoding's tensor.  f0, vuv, the voicing gate and the frame times are carried over:
        the result is ready for expand(wb) -> decode_device.  An encoding of line spectral frequencies takes ``lsf``
        instead of ``mcep`` (the other one is a ValueError): the p + 1 columns are generated, then the angles are
        repaired with ``min_gap`` > 0 radians (world.lsf.repair_device) — a generated track is not ordered."""
        from .dynamics import HTS_WINDOWS, compact_with_trajectories
        return compact_with_trajectories(self, mcep, band_ap, HTS_WINDOWS if windows is None else windows, lsf, min_gap)

    def align(self, other, radius=None):
        """world.align.align_compact(self, other, radius): dynamic time warping against another resident CompactEncoding of
        the same sentences, over the mel-cepstral coefficients 1 .. n0-1 or the p angles — no spectrogram is needed."""
        from .align import align_compact
        return align_compact(self, other, radius)

    # ---- files (host only) -------------------------------------------------------------------------------------------
    def save_npz(self, path):
        """One .npz for the batch: the tensors, the per-utterance frame offsets and the parameters."""
        h = self.to_host()
        out = {k: np.asarray(a) for k, a in h._tensors()}
        out["frame_off"] = h.frame_off
        out["fs"] = np.asarray(h.fs)
        out["fft_size"] = np.asarray(h.fft_size)
        out["frame_period"] = np.asarray(np.nan if h.frame_period is None else h.frame_period, dtype=np.float64)
        out["is_requiem"] = np.asarray(h.is_requiem)
        out["n0"] = np.asarray(-1 if h.n0 is None else int(h.n0))
        out["lowhz"] = np.asarray(h.lowhz, dtype=np.float64)
        out["highhz"] = np.asarray(h.highhz, dtype=np.float64)
        out["mcep_fs"] = np.asarray(-1 if h.mcep_fs is None else h.mcep_fs)
        if h.lsf is not None:  # (a file without the key is one of the other two kinds: files written before load as they did)
            out["lsf_order"] = np.asarray(h.lsf_order)
        np.savez(path, **out)

    @classmethod
    def load_npz(cls, path):
        with np.load(path) as z:
            g = {k: z[k] for k in z.files}
        n0 = int(g["n0"])
        fp = float(g["frame_period"])
        fs = g["fs"].item()
        return cls(None, fs, int(g["fft_size"]), None if np.isnan(fp) else (int(fp) if fp == int(fp) else fp),
                   bool(g["is_requiem"]), None if n0 < 0 else n0, g["lowhz"].item(), g["highhz"].item(), g["frame_off"],
                   g["temporal_positions"], g["f0"], g["vuv"], g.get("mcep"), g["band_ap"], g.get("ap_gate"),
                   g.get("spectrogram"), tp_host=g["temporal_positions"],
                   mcep_fs=None if g["mcep_fs"].item() == -1 else g["mcep_fs"].item(), lsf=g.get("lsf"),
                   lsf_order=int(g["lsf_order"]) if "lsf_order" in g else None)

    # ---- plain dicts (World.encode_compact_batch / decode_compact_batch) ---------------------------------------------
    def to_dicts(self):
        """Per utterance a small plain dict: f0, vuv, temporal_positions (frames,), mcep (frames, n0) as encode_mcep
        returns it, coarse_ap (bands, frames) as d4c() returns it (Requiem: d4cRequiem's 'aperiodicity' rows), ap_gate
        (frames,) (Requiem: None), fs, fft_size, is_requiem."""
        h = self.to_host()
        out = []
        for u in range(h.n_utt):
            s = slice(int(h.frame_off[u]), int(h.frame_off[u + 1]))
            d = {"f0": h.f0[s].copy(), "vuv": h.vuv[s].copy(), "temporal_positions": h.temporal_positions[s].copy(),
                 "coarse_ap": np.ascontiguousarray(h.band_ap[s].T),
                 "ap_gate": None if h.ap_gate is None else h.ap_gate[s].copy(),
                 "fs": h.fs, "fft_size": h.fft_size, "is_requiem": h.is_requiem}
            if h.mcep is not None:
                d["mcep"] = h.mcep[s].copy()
            elif h.lsf is not None:
                d["lsf"] = h.lsf[s].copy()
            else:
                d["spectrogram"] = np.ascontiguousarray(h.spectrogram[s].T)
            out.append(d)
        return out

    @classmethod
    def _from_lsf_dicts(cls, dats):
        d0 = dats[0]
        fs, fft_size, req = d0["fs"], int(d0["fft_size"]), bool(d0["is_requiem"])
        p = int(np.shape(d0["lsf"])[1]) - 1 if np.ndim(d0["lsf"]) == 2 else None
        _, nap = d4c_band_layout(fs, req)
        bands = nap + 2 if req else nap
        for n, d in enumerate(dats):
            if d["fs"] != fs or int(d["fft_size"]) != fft_size or bool(d["is_requiem"]) != req:
                raise ValueError("dict %d: the dicts of one batch must share fs, fft_size and is_requiem" % n)
            nf = len(d["f0"])
            per_frame = [("temporal_positions", (nf,)), ("f0", (nf,)), ("vuv", (nf,)), ("coarse_ap", (bands, nf)),
                         ("lsf", (nf, None if p is None else p + 1))]
            if not req:
                per_frame.append(("ap_gate", (nf,)))
            for key, shape in per_frame:
                if key not in d or d[key] is None or np.shape(d[key]) != shape:
                    raise ValueError("dict %d: '%s' must have shape %s, got %s"
                                     % (n, key, shape, None if d.get(key) is None else np.shape(d[key])))
        cat = lambda key, t=False: np.concatenate(  # noqa: E731
            [np.asarray(d[key], dtype=np.float64).T if t else np.asarray(d[key], dtype=np.float64) for d in dats])
        tp = cat("temporal_positions")
        frame_off = np.concatenate([[0], np.cumsum([len(d["f0"]) for d in dats])])
        return cls(None, fs, fft_size, None, req, None, 0, 8000, frame_off, tp, cat("f0"), cat("vuv"), None, cat("coarse_ap", True), None if req else cat("ap_gate"), None,
                   tp_host=tp, lsf=cat("lsf"), lsf_order=p)

    @classmethod
    def from_dicts(cls, dats):
        """Host encoding from to_dicts()-style dicts; raises ValueError for arrays whose lengths disagree and for dicts of
        mixed fs / fft_size / is_requiem / coefficient count.  Touches no device."""
        if not dats:
            raise ValueError("CompactEncoding.from_dicts: no dicts")
        d0 = dats[0]
        fs, fft_size, req = d0["fs"], int(d0["fft_size"]), bool(d0["is_requiem"])
        if "lsf" in d0:
            return cls._from_lsf_dicts(dats)
        coded = "mcep" in d0
        n0 = int(np.shape(d0["mcep"])[1]) if coded and np.ndim(d0["mcep"]) == 2 else None
        check_compact_args(fs, fft_size, n0 if coded else None, "CompactEncoding.from_dicts")
        _, nap = d4c_band_layout(fs, req)
        bands = nap + 2 if req else nap
        for n, d in enumerate(dats):
            if d["fs"] != fs or int(d["fft_size"]) != fft_size or bool(d["is_requiem"]) != req:
                raise ValueError("dict %d: the dicts of one batch must share fs, fft_size and is_requiem (%r / %r / %r "
                                 "against %r / %r / %r)" % (n, d["fs"], d["fft_size"], bool(d["is_requiem"]), fs, fft_size, req))
            nf = len(d["f0"])
            per_frame = [("temporal_positions", (nf,)), ("f0", (nf,)), ("vuv", (nf,)), ("coarse_ap", (bands, nf))]
            if not req:
                per_frame.append(("ap_gate", (nf,)))
            per_frame.append(("mcep", (nf, n0)) if coded else ("spectrogram", (fft_size // 2 + 1, nf)))
            for key, shape in per_frame:
                if key not in d or d[key] is None or np.shape(d[key]) != shape:
                    raise ValueError("dict %d: '%s' must have shape %s, got %s"
                                     % (n, key, shape, None if d.get(key) is None else np.shape(d[key])))
        cat = lambda key, t=False: np.concatenate(  # noqa: E731
            [np.asarray(d[key], dtype=np.float64).T if t else np.asarray(d[key], dtype=np.float64) for d in dats])
        frame_off = np.concatenate([[0], np.cumsum([len(d["f0"]) for d in dats])])
        tp = cat("temporal_positions")
        return cls(None, fs, fft_size, None, req, n0, 0, 8000, frame_off, tp, cat("f0"), cat("vuv"),
                   cat("mcep") if coded else None, cat("coarse_ap", True), None if req else cat("ap_gate"),
                   None if coded else cat("spectrogram", True), tp_host=tp)


def _bands_of(enc):
    if enc.is_requiem:
        return enc.aperiodicity, None
    band_ap, gate = getattr(enc, "coarse_ap", None), getattr(enc, "ap_gate", None)
    if band_ap is None or gate is None:
        raise ValueError("compact: this encoding holds no band aperiodicity: encode with want_coarse=True")
    return band_ap, gate


def _compact_lsf(enc, lsf_order):
    """compact(lsf_order=p): the spectrum as line spectral frequencies, at any sampling rate."""
    from .lsf import check_order, lsf_device
    p = check_order(lsf_order, "compact", enc.fft_size // 2 + 1)
    band_ap, gate = _bands_of(enc)
    rt = enc.rt
    with rt.lock, rt.on_stream():
        rows = lsf_device(rt, enc.spectrogram, p)
    return CompactEncoding(rt, enc.fs, enc.fft_size, enc.frame_period, enc.is_requiem, None, 0, 8000, enc.batch.frame_off,
                           enc.temporal_positions, enc.f0, enc.vuv, None, band_ap, gate, None, tp_host=enc.tp_host,
                           lsf=rows, lsf_order=p)


def compact_encoding(enc, n0=40, lowhz=0, highhz=8000, mcep_fs=None, lsf_order=None):
    """BatchEncoding.compact: see there."""
    if lsf_order is not None:
        return _compact_lsf(enc, lsf_order)
    mcep_fs = enc.fs if mcep_fs is None else mcep_fs
    check_compact_args(mcep_fs, enc.fft_size, n0, "compact")
    rt = enc.rt
    if enc.is_requiem:
        band_ap, gate = enc.aperiodicity, None
    else:
        band_ap, gate = getattr(enc, "coarse_ap", None), getattr(enc, "ap_gate", None)
        if band_ap is None or gate is None:
            raise ValueError("compact: this encoding holds no band aperiodicity: encode with want_coarse=True")
    mcep = spec = None
    if n0 is None:
        spec = enc.spectrogram
    else:
        from .features import mcep_device
        with rt.lock, rt.on_stream():
            mcep = mcep_device(rt, enc.spectrogram, int(n0), mcep_fs, lowhz, highhz)
    return CompactEncoding(rt, enc.fs, enc.fft_size, enc.frame_period, enc.is_requiem, None if n0 is None else int(n0),
                           lowhz, highhz, enc.batch.frame_off, enc.temporal_positions, enc.f0, enc.vuv, mcep, band_ap, gate,
                           spec, tp_host=enc.tp_host, mcep_fs=mcep_fs)
