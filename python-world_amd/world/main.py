"""`World` facade: the class, method names, argument order / defaults and result-dict keys of the reference's
world/main.py:26-214, with every stage running on the MI355X through libworld_hip.so.

The analysis/synthesis path, the spectral feature heads that follow encode() (mel filterbank energies, mel-cepstrum
and its inverse, context stacking: world/features.py) and the manifold vocoder's networks (encode_vae:
world/manifold.py) are provided; the reference's plotting (draw) is not part of this build.
"""
import logging
import os

import numpy as np

from . import _hip
from . import cheaptrick as _ct
from . import d4c as _d4c
from . import d4cRequiem as _d4cr
from . import features as _feat
from . import manifold as _man
from . import dio as _dio
from . import get_seeds_signals as _seeds
from . import harvest as _hv
from . import stonemask as _sm
from . import swipe as _swipe
from . import synthesis as _syn
from . import synthesisRequiem as _synr

_SOURCE_KEYS = ('temporal_positions', 'vuv', 'f0')


def _pick(d, keys):
    return {k: d[k] for k in keys}


def _estimate_source(fs, x, method, floor, ceil, channels, target_fs, period, allowed_range):
    """F0 stage shared by get_f0 / get_spectrum / encode (world/main.py:36-46, 62-72, 121-135).  allowed_range is None
    for the two getters, which call dio() positionally without it."""
    if np.ndim(x) != 1:
        raise ValueError("the waveform must be 1-D (one channel), got shape %s" % (np.shape(x),))
    if method == 'dio':
        extra = {} if allowed_range is None else {'allowed_range': allowed_range}
        source = _dio.dio(x, fs, floor, ceil, channels, target_fs, period, **extra)
        source['f0'] = _sm.stonemask(x, fs, source['temporal_positions'], source['f0'])
        return source
    if method == 'harvest':
        return _hv.harvest(x, fs, f0_floor=floor, f0_ceil=ceil, frame_period=period)
    if method == 'swipe':
        return _swipe.swipe(fs, x, plim=[floor, ceil], sTHR=0.3)
    raise Exception  # the reference raises a bare Exception for an unknown method


def _aperiodicity(x, fs, source, fft_size, is_requiem):
    if is_requiem:
        return _d4cr.d4cRequiem(x, fs, source, fft_size=fft_size)
    return _d4c.d4c(x, fs, source, fft_size_for_spectrum=fft_size)


# World.encode_batch / decode_batch cut a batch of at least this many bytes of waveform (audio to be rendered) into two
# parts that run on two pipelines, so that one part's PCIe transfer lies under the other's kernels
FACADE_SPLIT_BYTES = int(os.environ.get("WH_FACADE_SPLIT_BYTES", str(16 << 20)))
FACADE_LANE = int(os.environ.get("WH_FACADE_LANE", "2001"))  # the pipelines the parts run on: lane ids (contexts, flags, streams) no public class hands out, so the
# facade's flag reads never consume — or raise for — a condition of the caller's own WorldBatchPipeline / WorldBatchLanes
# work in flight
# (Measured and not kept: the later part's stream at high priority, and its decode time base computed ahead under the
# earlier part's responses — 23.0 ... 24.6 ms against 23.4 for the resynthesis flow of 64 x 10 s, within the noise.)


def _decode_groups(dats, kw):
    """Consecutive [start, end) parts of a decode_batch list: one part for small batches, for Requiem (its noise cursor
    runs through the utterances in order) and for a caller that steers the checks itself; otherwise two — cut where the
    list passes from one resident encoding to the next if it does so exactly once (the two halves of encode_batch: each
    keeps its tensors as they are), else balanced by frames."""
    from .distributed import shard_ranges

    n = len(dats)
    if n < 2 or bool(dats[0]['is_requiem']) or any(k in kw for k in ('seeds', 'cursor', 'check')):
        return [(0, n)]
    frames = [len(d['f0']) for d in dats]
    seconds = sum(float(d['temporal_positions'][-1]) for d in dats if len(d['temporal_positions']))
    if 8 * seconds * dats[0]['fs'] < FACADE_SPLIT_BYTES:  # the audio to be rendered
        return [(0, n)]
    encs = [getattr(d, '_enc', None) for d in dats]
    cuts = [i for i in range(1, n) if encs[i] is not encs[i - 1]]
    if len(cuts) == 1:
        return [(0, cuts[0]), (cuts[0], n)]
    return [(a, b) for a, b in shard_ranges(frames, 2) if b > a]


def _hand_out(dats, block, y_off, copy_out):
    """d['out'] for every dict from the batch's host block (page-locked): arrays of their own in pageable memory — the
    copies run on the staging pool's threads, NumPy releases the GIL for them — or, ``copy_out=False``, views."""
    cuts = [(int(y_off[u]), int(y_off[u + 1])) for u in range(len(dats))]
    if not copy_out:
        for d, (a, b) in zip(dats, cuts):
            d['out'] = block[a:b]
        return
    if block.nbytes < (1 << 22) or len(dats) < 4:
        outs = [np.array(block[a:b]) for a, b in cuts]
    else:
        # (allocating the arrays on this thread and only filling them in the pool was measured and is worse: 49 against
        # 28 - 39 ms for the 164 MB of a 64 x 20 s batch; the views of copy_out=False: 23 ms)
        with _hip._copy_pool() as pool:
            outs = list(pool.map(lambda ab: np.array(block[ab[0]:ab[1]]), cuts))
    for d, y in zip(dats, outs):
        d['out'] = y


def _check_decodable(dats):
    """What decode() / decode_batch() are handed: the per-frame arrays of a dict must agree in length and the dense tensors
    be (bins, frames) over those frames; the dicts of one batch must share rate, synthesis path and bin count.  The
    reference fails somewhere inside NumPy on such input (an interp1d shape error, a broadcast error); here the kernels
    index by the batch's frame count, so a short array would be read past its end — refused up front instead.  Dense values
    still resident in HBM (lazy dicts) are what encode made: not looked at, not materialised."""
    fs0 = req0 = k0 = None
    for n, d in enumerate(dats):
        tp, f0, vuv = (np.asarray(d[k]) for k in ('temporal_positions', 'f0', 'vuv'))
        if not (tp.ndim == f0.ndim == vuv.ndim == 1 and len(tp) == len(f0) == len(vuv)):
            raise ValueError("dict %d: temporal_positions / f0 / vuv must be 1-D and of one length (%s, %s, %s)"
                             % (n, tp.shape, f0.shape, vuv.shape))
        if len(tp) < 2:
            raise ValueError("dict %d: fewer than 2 frames" % n)
        for key in ('spectrogram', 'aperiodicity'):
            v = dict.get(d, key)
            if isinstance(v, np.ndarray) and (v.ndim != 2 or v.shape[1] != len(tp)):
                raise ValueError("dict %d: '%s' must be (bins, %d frames), got %s" % (n, key, len(tp), v.shape))
        sp = dict.get(d, 'spectrogram')
        k = sp.shape[0] if isinstance(sp, np.ndarray) else None
        if fs0 is None:
            fs0, req0 = d['fs'], bool(d['is_requiem'])
        elif d['fs'] != fs0 or bool(d['is_requiem']) != req0:
            raise ValueError("dict %d: the dicts of one decode_batch must share fs and is_requiem (%s / %s against %s / %s)"
                             % (n, d['fs'], bool(d['is_requiem']), fs0, req0))
        if k is not None:
            if k0 is None:
                k0 = k
            elif k != k0:
                raise ValueError("dict %d: spectrogram of %d bins in a batch of %d" % (n, k, k0))


def _vae_args(x, energy, n0, mean, window):
    """encode_vae / decode_vae's arguments, checked before anything is touched: (energy, mean as n0-1 values, window)."""
    n0, window = int(n0), int(window)
    if np.ndim(x) != 2:
        raise ValueError("encode_vae: the input must be (frames, coefficients), got shape %s" % (np.shape(x),))
    energy = np.asarray(energy, dtype=np.float64).reshape(-1)
    if energy.shape[0] != x.shape[0]:
        raise ValueError("encode_vae: energy has %d values for %d frames" % (energy.shape[0], x.shape[0]))
    if n0 < 2 or window < 0:
        raise ValueError("encode_vae: n0 must be >= 2 and window >= 0")
    try:
        m = np.ascontiguousarray(np.broadcast_to(np.asarray(mean, dtype=np.float64), (n0 - 1,)))
    except ValueError:
        raise ValueError("encode_vae: mean must broadcast to the %d coefficients, got shape %s" % (n0 - 1, np.shape(mean)))
    return energy, n0, m, window


class World(object):
    # ---- analysis -----------------------------------------------------------------------------------------
    def get_f0(self, fs, x, f0_method='harvest', f0_floor=71, f0_ceil=800, channels_in_octave=2, target_fs=4000,
               frame_period=5):
        """(temporal_positions, f0, vuv) — world/main.py:27-49."""
        s = _estimate_source(fs, x, f0_method, f0_floor, f0_ceil, channels_in_octave, target_fs, frame_period, None)
        return tuple(s[k] for k in ('temporal_positions', 'f0', 'vuv'))

    def get_spectrum(self, fs, x, f0_method='harvest', f0_floor=71, f0_ceil=800, channels_in_octave=2,
                     target_fs=4000, frame_period=5, fft_size=None):
        """world/main.py:51-79."""
        s = _estimate_source(fs, x, f0_method, f0_floor, f0_ceil, channels_in_octave, target_fs, frame_period, None)
        env = _ct.cheaptrick(x, fs, s, fft_size=fft_size)
        out = _pick(s, ('f0', 'temporal_positions'))
        out['fs'] = fs
        out.update(_pick(env, ('ps spectrogram', 'spectrogram')))
        return out

    def encode_w_gvn_f0(self, fs, x, source, fft_size=None, is_requiem=False):
        """world/main.py:81-104, quirks included: fft_size=None raises TypeError at the assert and is_requiem=True
        raises KeyError('coarse_ap')."""
        assert np.all(source['f0'] >= 3 * fs / fft_size)
        env = _ct.cheaptrick(x, fs, source, fft_size=fft_size)
        source = _aperiodicity(x, fs, source, fft_size, is_requiem)
        out = _pick(source, _SOURCE_KEYS)
        out['fs'] = fs
        out['spectrogram'] = env['spectrogram']
        out.update(_pick(source, ('aperiodicity', 'coarse_ap')))
        out['is_requiem'] = is_requiem
        return out

    def encode(self, fs, x, f0_method='harvest', f0_floor=71, f0_ceil=800, channels_in_octave=2, target_fs=4000,
               frame_period=5, allowed_range=0.1, fft_size=None, is_requiem=False):
        """world/main.py:106-152."""
        if fft_size != None:  # noqa: E711 — the reference's own test: 0 also counts as "given"
            f0_floor = 3.0 * fs / fft_size
        source = _estimate_source(fs, x, f0_method, f0_floor, f0_ceil, channels_in_octave, target_fs, frame_period,
                                  allowed_range)
        env = _ct.cheaptrick(x, fs, source, fft_size=fft_size)
        source = _aperiodicity(x, fs, source, fft_size, is_requiem)
        out = _pick(source, ('temporal_positions', 'vuv'))
        out['fs'] = env['fs']
        out.update(_pick(source, ('f0', 'aperiodicity')))
        out.update(_pick(env, ('ps spectrogram', 'spectrogram')))
        out['is_requiem'] = is_requiem
        return out

    # ---- batched convenience (not in the reference; SURVEY.md §8(b): "World.encode_batch/decode_batch") ----------
    @_hip.serialised
    def encode_batch(self, fs, xs, f0_method='harvest', f0_floor=71, f0_ceil=800, channels_in_octave=2, target_fs=4000,
                     frame_period=5, allowed_range=0.1, fft_size=None, is_requiem=False, want_ps=False, devices=None):
        """encode() — same arguments, same defaults (Harvest) — for a list of utterances in one pass per kernel.
        ``devices``: a list of GPU indices — the batch is cut into contiguous ranges balanced by samples and every range
        runs on its device from a host thread of its own (``world.pool.WorldBatchPool``: one process, no
        torch.distributed); the dicts are the single-device ones, bit for bit.
        Each dict has encode()'s keys; 'ps spectrogram' (the complex pitch-synchronous spectra of world/main.py:149,
        fft_size x frames x 16 B per utterance) only with ``want_ps=True``.  Under an initialised
        torch.distributed process group (one process per GPU) the batch is sharded by utterance over the ranks and the
        list holds only this rank's utterances; use ``world.distributed.ShardedWorldBatch`` directly to keep results
        on the device.

        The dicts are ``world.batch.EncodingDict``s: real dicts whose dense values ('spectrogram', 'aperiodicity',
        'ps spectrogram') are downloaded when first read; ``decode_batch`` takes whatever was never read straight from
        HBM.  ``encode_batch -> scale_pitch -> scale_duration -> decode_batch`` moves no dense tensor over PCIe."""
        from .batch import WorldBatchPipeline
        from .distributed import ShardedWorldBatch, shard_ranges

        kw = dict(f0_method=f0_method, f0_floor=f0_floor, f0_ceil=f0_ceil, channels_in_octave=channels_in_octave,
                  target_fs=target_fs, frame_period=frame_period, allowed_range=allowed_range, fft_size=fft_size,
                  is_requiem=is_requiem, want_ps=want_ps)
        if devices is not None:
            from .pool import WorldBatchPool
            dats = WorldBatchPool.shared(devices).encode(list(xs), fs, **kw).to_dicts(want_ps=want_ps, lazy=True)
            for d in dats:
                d['_batch_range'] = (0, len(dats))
            return dats
        sb = ShardedWorldBatch()
        lo, hi = sb.shard([len(x) for x in xs])
        mine = list(xs[lo:hi])
        if len(mine) >= 2 and 8 * sum(len(x) for x in mine) >= FACADE_SPLIT_BYTES:
            # Two halves on two pipelines (contexts and streams of their own): the second half's waveforms cross PCIe
            # under the first half's kernels.  Utterances are independent and every stage numbers its work per
            # utterance, so the dicts are the ones the single batch gives, bit for bit.
            pipe = WorldBatchPipeline(sb.backend.rt.index, depth=2, prefetch_timebase=False, first_lane=FACADE_LANE)
            parts = [(a, b) for a, b in shard_ranges([len(x) for x in mine], 2) if b > a]
            wbs = [pipe.next() for _ in parts]
            encs = [wb.encode(mine[a:b], fs, check=False, **kw) for wb, (a, b) in zip(wbs, parts)]
            pipe.synchronize(check=False)
            err = None
            for i, wb in enumerate(wbs):  # every part's flags are read (and a Harvest part that needs it repeated), then the first error raised
                try:
                    encs[i] = wb.settle_encode(encs[i], "World.encode_batch")
                except _hip.WorldHipError as e:
                    err = err or e
            if err is not None:
                raise err
            dats = [d for e in encs for d in e.to_dicts(want_ps=want_ps, lazy=True)]
        else:
            enc = sb.encode(xs, fs, **kw)
            dats = enc.to_dicts(want_ps=want_ps, lazy=True) if enc is not None else []
        for d in dats:
            d['_batch_range'] = sb.range
        return dats

    @_hip.serialised
    def decode_batch(self, dats, devices=None, copy_out=True, **kw):
        """decode() for a list of encode()/encode_batch() dicts that share fs / is_requiem / fft size: one batched
        synthesis; adds 'out' to every dict (peak-normalised like decode()) and returns the list.
        ``devices``: as in encode_batch — one host thread per listed GPU, each decoding a contiguous range (dicts that
        encode_batch(devices=...) made go back to the device that holds them); same samples as the single batch.
        ``copy_out`` (default): every 'out' is an array of its own in pageable memory, as decode() returns it;
        False: views into ONE page-locked block per batch (part) — no host copy, but a caller that keeps a single
        utterance keeps the whole batch's block locked.
        Randomness differs from decode() unless asked otherwise: the noise comes from the device Philox stream
        (``seed=``) and Requiem batches use device-built seed tables with the noise cursor restarted at 0 on every
        call, whereas decode() draws from NumPy's global stream / get_seeds_signals() and keeps
        ``synthesisRequiem.generate_noise.current_index`` across calls.  For sample-comparable output pass
        ``noise=[randn arrays]`` (pulse-wise) or ``seeds=get_seeds_signals(fs), cursor=...`` (Requiem): keywords of
        ``WorldBatch.decode_device``."""
        from .batch import BatchEncoding, WorldBatch

        if not dats:
            return dats
        _check_decodable(dats)
        if devices is not None:
            from .pool import WorldBatchPool
            for d, y in zip(dats, WorldBatchPool.shared(devices).decode_dicts(dats, **kw)):
                d['out'] = y
            return dats
        groups = _decode_groups(dats, kw)
        if len(groups) > 1:
            return self._decode_batch_parts(dats, groups, kw, copy_out)
        wb = WorldBatch()
        enc = BatchEncoding.from_dicts(wb.rt, dats)
        y, y_off = wb.decode_device(enc, **kw)
        with wb.rt.on_stream():
            y = wb.rt.to_host(y)  # one pinned block
        _hand_out(dats, y, y_off, copy_out)
        return dats

    def _decode_batch_parts(self, dats, groups, kw, copy_out=True):
        """decode_batch with the batch cut into consecutive parts, each on a pipeline of its own (context, stream): part
        g + 1 renders behind part g's kernels, so part g's audio crosses PCIe under them.  Same samples as the single
        batch: the overlap-add runs are numbered per utterance and the Philox stream of utterance u is re-keyed to its
        index in the whole list (synthesis.philox_seed_for_offset)."""
        from .batch import BatchEncoding, WorldBatch

        noise, seed = kw.get('noise'), kw.get('seed', 0)
        index = WorldBatch().rt.index
        pend, prev, wb = [], None, None
        try:
            for g, (a, b) in enumerate(groups):
                wb = WorldBatch(index, lane=FACADE_LANE + g, prefetch_timebase=False)
                rt, torch = wb.rt, wb.rt.torch
                enc = BatchEncoding.from_dicts(rt, dats[a:b])
                kw_g = dict(kw, seed=_syn.philox_seed_for_offset(seed, a), check=False)
                if noise is not None:
                    kw_g['noise'] = noise[a:b]
                if prev is not None:
                    rt.own_stream.wait_event(prev)
                y, y_off = wb.decode_device(enc, **kw_g)
                with rt.on_stream():
                    prev = torch.cuda.Event()
                    prev.record(torch.cuda.current_stream(rt.device))
                    host = torch.empty(y.shape, dtype=y.dtype, pin_memory=True)
                    nbytes = y.numel() * y.element_size()
                    if g + 1 < len(groups) and y.is_contiguous() and nbytes % 8 == 0:
                        # a few workgroups write the pinned block through its device mapping.  (The runtime's own
                        # D2H copy is a chip-wide kernel whose waves sit on PCIe: the next part's kernels made no
                        # progress under it — rocprofv3 trace: its first 0.05 ms kernel ended when the 1.5 ms copy did.)
                        _hip.check(rt.lib.wh_copy_mapped(rt.ctx, rt.stream(), _hip._vp(host.data_ptr()), rt.ptr(y),
                                                         nbytes, 16))
                    else:
                        host.copy_(y, non_blocking=True)
                pend.append((wb, enc, kw_g, y, y_off, host))
        except BaseException:
            # nothing of an abandoned batch is left standing in the pipelines' contexts: the parts in flight AND the part
            # whose enqueueing failed (its stream may hold half a decode, its flags a condition of it)
            for w in {id(w): w for w in [p[0] for p in pend] + ([wb] if wb is not None else [])}.values():
                try:
                    w.rt.own_stream.synchronize()
                    w.rt.take_flags()
                except _hip.WorldHipError:
                    pass
            raise
        for wb, *_ in pend:
            wb.rt.own_stream.synchronize()
        settled, err = [], None
        for wb, enc, kw_g, y, y_off, host in pend:  # (every part's conditions are read, whichever raises)
            try:
                settled.append(wb.settle_decode(enc, (y, y_off), **kw_g))
            except _hip.WorldHipError as e:
                settled.append(None)
                err = err or e
        if err is not None:
            raise err
        for (a, b), (wb, enc, kw_g, y, y_off, host), (y2, y_off2) in zip(groups, pend, settled):
            out = host.numpy()
            if y2 is not y:  # rendered again with the safe pulse capacity
                with wb.rt.on_stream():
                    out = wb.rt.to_host(y2)
            _hand_out(dats[a:b], out, y_off2, copy_out)
        return dats

    @_hip.serialised
    def encode_batch_w_gvn_f0(self, fs, xs, sources, fft_size=None, is_requiem=False, devices=None):
        """encode_w_gvn_f0 (world/main.py:81-104) for a list of utterances in one pass per kernel: ``sources[u]`` is the
        dict with 'temporal_positions', 'f0' and 'vuv' that goes with ``xs[u]``.  A source whose temporal_positions are
        the batch's own 5 ms grid is taken as it is; any other — a 10 ms tracker, a laryngograph's time stamps — is
        interpolated onto the grid on the device with the voiced rule (BatchEncoding.set_pitch_contour).  Returns a list
        of dicts with encode_w_gvn_f0's keys and that utterance's values, bit for bit; a Requiem dict has no
        'coarse_ap' (the reference raises KeyError there: SURVEY Q16).  The reference's quirks stay: the assert on every
        source's f0, TypeError for fft_size=None.  The sources are not modified."""
        from .batch import WorldBatch
        from .regrid import interp_contour_device, knot_lists

        if devices is not None:
            raise NotImplementedError("encode_batch_w_gvn_f0(devices=...): run one WorldBatch per device instead")
        xs, sources = list(xs), list(sources)
        if len(sources) != len(xs):
            raise ValueError("encode_batch_w_gvn_f0: %d sources for %d utterances" % (len(sources), len(xs)))
        for source in sources:
            assert np.all(source['f0'] >= 3 * fs / fft_size)
            _hip.same_frames("encode_batch_w_gvn_f0", temporal_positions=source['temporal_positions'], f0=source['f0'],
                             vuv=source['vuv'])
        if not xs:
            return []
        wb = WorldBatch()
        rt = wb.rt
        batch, x_d, tp_d = wb.upload(xs, fs)
        fo = batch.frame_off
        grid = [batch.tp_host[int(fo[u]):int(fo[u + 1])] for u in range(len(xs))]
        as_is = [np.array_equal(np.asarray(s['temporal_positions'], dtype=np.float64), g) for s, g in zip(sources, grid)]
        f64 = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
        with rt.lock, rt.on_stream():
            if all(as_is):
                scal = rt.to_device_concat([f64(s[k]) for k in ('f0', 'vuv') for s in sources]).view(2, -1)
                f0_d, vuv_d = scal[0], scal[1]
            else:
                # (a source on the grid passes through the exact-hit rule value for value; its vuv is the caller's to
                # say, so those utterances' slices are overwritten with what was passed)
                off, t, v = knot_lists([s['temporal_positions'] for s in sources], [s['f0'] for s in sources], len(xs),
                                       "encode_batch_w_gvn_f0")
                f0_d, vuv_d = interp_contour_device(rt, batch, tp_d, off, t, v, True)
                for u, s in enumerate(sources):
                    if as_is[u]:
                        f0_d[int(fo[u]):int(fo[u + 1])] = rt.to_device(f64(s['f0']))
                        vuv_d[int(fo[u]):int(fo[u + 1])] = rt.to_device(f64(s['vuv']))
        enc = wb.encode_given_f0(batch, x_d, tp_d, fs, f0_d, vuv_d, fft_size=fft_size, is_requiem=is_requiem,
                                 want_coarse=not is_requiem)
        dats = enc.to_dicts()
        with rt.lock, rt.on_stream():
            coarse = None if is_requiem else [rt.to_host(enc.coarse_ap[int(fo[u]):int(fo[u + 1])], transpose=True)
                                              for u in range(len(xs))]
        out = []
        for u, d in enumerate(dats):
            o = _pick(d, _SOURCE_KEYS)
            o['fs'] = fs
            o['spectrogram'] = d['spectrogram']
            o['aperiodicity'] = d['aperiodicity']
            if not is_requiem:
                o['coarse_ap'] = coarse[u]
            o['is_requiem'] = is_requiem
            out.append(o)
        return out

    # ---- compact encodings (not in the reference's class; world/compact.py) --------------------------------------
    @_hip.serialised
    def encode_compact_batch(self, fs, xs, n0=40, devices=None, **encode_kw):
        """encode_batch() whose results leave the GPU in their compact form: per utterance a small plain dict with f0, vuv,
        temporal_positions, the n0-coefficient mel-cepstrum 'mcep' (frames, n0) that encode_mcep(spectrogram.T, n0) gives
        (test/spectralFeatures.py:31-33), D4C's band aperiodicity 'coarse_ap' (bands, frames) (world/d4c.py:57,62) with
        its voicing gate 'ap_gate' (frames,), fs, fft_size and is_requiem — 360 B per frame at 16 kHz instead of the 8 232
        of the dense tensors, none of which crosses PCIe.  ``encode_kw``: encode_batch's keywords (Harvest by default).
        Requiem encodings carry d4cRequiem's band rows under 'coarse_ap' and no gate.  fs must be 16000: decode_mcep
        hard-codes it (world/main.py:347-355)."""
        from .batch import WorldBatch
        from .cheaptrick import default_fft_size
        from .compact import check_compact_args

        if n0 is None:
            raise ValueError("encode_compact_batch: n0=None (dense spectrogram kept) is BatchEncoding.compact(n0=None)'s job")
        fft_size = encode_kw.get('fft_size')
        check_compact_args(fs, int(fft_size) if fft_size is not None else default_fft_size(fs), n0, "encode_compact_batch")
        if devices is not None:
            raise NotImplementedError("encode_compact_batch(devices=...): world.pool hands back one merged encoding per "
                                      "call, not per-device ones to compact; run one WorldBatch per device instead")
        xs = list(xs)
        if not xs:
            return []
        kw = dict(encode_kw)
        kw.setdefault('f0_method', 'harvest')
        wb = WorldBatch()
        enc = wb.encode(xs, fs, want_coarse=not kw.get('is_requiem', False), **kw)
        return enc.compact(n0).to_dicts()

    @_hip.serialised
    def decode_compact_batch(self, dats, devices=None, **decode_kw):
        """decode_batch() for encode_compact_batch's dicts: the compact arrays are uploaded as one block, expanded on the
        device (decode_mcep's kernel for the spectrogram, wh_aperiodicity_from_bands for the aperiodicity — D4C's own
        rows, bit for bit) and synthesised in one batch; adds 'out' to every dict and returns the list.  ``decode_kw``:
        keywords of WorldBatch.decode_device (``seed=``, ``noise=``, ...)."""
        from .batch import WorldBatch
        from .compact import CompactEncoding

        if not dats:
            return dats
        ce = CompactEncoding.from_dicts(dats)  # (every check before anything touches the device)
        for n, d in enumerate(dats):
            if len(d['f0']) < 2:
                raise ValueError("dict %d: fewer than 2 frames" % n)
        if devices is not None:
            raise NotImplementedError("decode_compact_batch(devices=...): run one WorldBatch per device instead")
        wb = WorldBatch()
        y, y_off = wb.decode_device(ce.expand(wb), **decode_kw)
        with wb.rt.on_stream():
            y = wb.rt.to_host(y)
        _hand_out(dats, y, y_off, True)
        return dats

    # ---- frame alignment of parallel utterances (not in the reference's class; world/align.py) -------------------
    @_hip.serialised
    def align(self, dat_a, dat_b, n0=40, lowhz=0, highhz=8000, radius=None):
        """Dynamic time warping of two encode() dicts of the same sentence over their mel-cepstra (encode_mcep with n0
        coefficients, the energy dropped), on the device: {'path_a', 'path_b'} frame indices into each dict, 'cost' the
        sum of the Euclidean local costs along the path and 'mcd' the aligned mel-cepstral distortion in dB.
        ``radius``: None or the half-width of a band around the diagonal."""
        from .align import align_dicts
        return align_dicts([dat_a], [dat_b], n0, lowhz, highhz, radius)[0]

    @_hip.serialised
    def align_batch(self, dats_a, dats_b, n0=40, lowhz=0, highhz=8000, radius=None, devices=None):
        """align() for lists of dicts, pair u aligning dats_a[u] with dats_b[u] in one batch: a list of result dicts."""
        from .align import align_dicts
        if devices is not None:
            raise NotImplementedError("align_batch(devices=...): run one WorldBatch per device instead")
        return align_dicts(dats_a, dats_b, n0, lowhz, highhz, radius)

    def warp_to(self, dat_a, dat_b, alignment):
        """dat_a on dat_b's timing: a new dict with dat_b's temporal_positions whose frame j holds dat_a's frame at the
        middle of the stretch that ``alignment`` (align()'s result for the two) pairs with j — f0, vuv, spectrogram and
        aperiodicity; decode() takes it."""
        from .align import warp_dict
        return warp_dict(dat_a, dat_b, alignment)

    # ---- dynamic features and parameter generation (not in the reference's class; world/dynamics.py) ---------------
    @_hip.serialised
    def delta_features(self, x, windows=None, devices=None):
        """Static + delta + delta-delta rows (any 1 .. 4 windows of half-width <= 2, the first the static one; default
        world.dynamics.HTS_WINDOWS) of one utterance x [T][d] or of a list of them, on the device: [T][n_win d], column
        w * d + c being window w over column c; a tap that reaches outside the utterance is dropped."""
        from .dynamics import HTS_WINDOWS, delta_features_numpy
        if devices is not None:
            raise NotImplementedError("delta_features(devices=...): run one WorldBatch per device instead")
        return delta_features_numpy(x, HTS_WINDOWS if windows is None else windows)

    @_hip.serialised
    def mlpg(self, mean, var, windows=None, devices=None):
        """Maximum-likelihood parameter generation: the track [T][d] that is most likely under the means [T][n_win d] and
        variances (the same shape, or one row [n_win d] for every frame) of its static and dynamic features — one
        utterance or a list of them, solved on the device (one banded LDL' per utterance and column)."""
        from .dynamics import HTS_WINDOWS, mlpg_numpy
        if devices is not None:
            raise NotImplementedError("mlpg(devices=...): run one WorldBatch per device instead")
        return mlpg_numpy(mean, var, HTS_WINDOWS if windows is None else windows)

    # ---- joint-density GMM voice conversion (not in the reference's class; world/gmm.py) ----------------------------
    @_hip.serialised
    def fit_conversion(self, dats_a, dats_b, n_components=8, n0=40, n_iter=20, devices=None, lsf_order=None, **kw):
        """A conversion model from parallel utterances: encode() dicts of a source speaker and of a target speaker, pair
        u the same sentence.  The pairs are aligned (align_batch's warping over mel-cepstra), the static + delta rows of
        the mel-cepstral coefficients 1 .. n0-1 of both sides are joined along the paths, and a mixture of
        ``n_components`` full-covariance Gaussians is fitted by ``n_iter`` EM iterations on the device
        (world.gmm.fit_device; ``kw``: reg_covar, seed, init, radius, windows, ...).  Returns a world.gmm.JointGMM.
        ``lsf_order`` = p (even, <= 40): the same over the p angles of line spectral frequencies (encode_lsf's rows, the
        gain dropped) instead of the mel-cepstrum — at any sampling rate; convert_voice follows the model's kind."""
        from .gmm import fit_conversion_dicts
        if devices is not None:
            raise NotImplementedError("fit_conversion(devices=...): run one WorldBatch per device instead")
        return fit_conversion_dicts(dats_a, dats_b, n_components, n0, n_iter, lsf_order=lsf_order, **kw)

    @_hip.serialised
    def convert_voice(self, dat, model, mode="mlpg", devices=None, **kw):
        """An encode() dict of the source speaker -> a new dict whose spectrogram is the target speaker's under
        ``model`` (fit_conversion's): maximum-likelihood trajectory conversion of the mel-cepstrum (``mode``: 'mlpg',
        'mmse' or 'frame'), coefficient 0, f0, vuv and aperiodicity carried over; decode() takes it."""
        from .gmm import convert_voice_dict
        if devices is not None:
            raise NotImplementedError("convert_voice(devices=...): run one WorldBatch per device instead")
        return convert_voice_dict(dat, model, mode, **kw)

    # ---- exemplar-based conversion: frame selection from the target's own frames (world/exemplar.py) -------------------
    @_hip.serialised
    def build_exemplars(self, dats_a, dats_b, n0=40, lsf_order=None, radius=None, devices=None, **kw):
        """A frame database from parallel utterances: encode() dicts of a source speaker and of a target speaker, pair u
        the same sentence.  The pairs are aligned as fit_conversion aligns them; row r of the database is target frame r
        (static + delta rows of the mel-cepstral coefficients 1 .. n0-1, or of the ``lsf_order`` angles) next to the
        source's rows at the aligned frame.  Returns a world.exemplar.FrameDatabase (``kw``: windows, normalise, ...)."""
        from .exemplar import build_exemplars_dicts
        if devices is not None:
            raise NotImplementedError("build_exemplars(devices=...): run one WorldBatch per device instead")
        return build_exemplars_dicts(dats_a, dats_b, n0, lsf_order, radius, **kw)

    @_hip.serialised
    def convert_voice_exemplar(self, dat, db, k=16, weight=1.0, mode="frames", devices=None, **kw):
        """An encode() dict of the source speaker -> a new dict whose spectrogram is made of frames the target speaker
        produced: for every frame the ``k`` database rows nearest on the source side, one of them chosen by a Viterbi
        pass whose concatenation cost is ``weight`` times the distance to what followed the previous choice in the
        target's recording.  ``mode`` 'frames': the chosen rows themselves; 'mlpg': a trajectory through their static
        and delta rows.  Coefficient 0, f0, vuv and aperiodicity are carried over; decode() takes it."""
        from .exemplar import convert_voice_exemplar_dict
        if devices is not None:
            raise NotImplementedError("convert_voice_exemplar(devices=...): run one WorldBatch per device instead")
        return convert_voice_exemplar_dict(dat, db, k, weight, mode, **kw)

    # ---- a per-frame spectral gain on a recording: vocoder-free conversion (world/specfilter.py) -----------------------
    @_hip.serialised
    def filter_waveform(self, fs, x, dat_num, dat_den=None, devices=None):
        """The recording ``x`` filtered frame by frame with the minimum-phase response of dat_num's spectrogram over
        dat_den's (encode() dicts on x's frame grid; ``dat_den`` None: of dat_num's alone): Hanning windows on the frame
        hop, overlap-added; excitation, phase and aperiodicity stay the recording's.  Not peak-normalised."""
        from .specfilter import filter_waveform_numpy
        if devices is not None:
            raise NotImplementedError("filter_waveform(devices=...): run one WorldBatch per device instead")
        return filter_waveform_numpy(fs, x, dat_num, dat_den)

    @_hip.serialised
    def convert_waveform(self, fs, x, dat, model, mode="mlpg", devices=None, **kw):
        """Vocoder-free voice conversion: ``x`` (the recording ``dat`` was encoded from) filtered by the converted over
        the source envelope under ``model`` (fit_conversion's), both as the model codes them; the source's f0 is kept."""
        from .gmm import convert_waveform_dict
        if devices is not None:
            raise NotImplementedError("convert_waveform(devices=...): run one WorldBatch per device instead")
        return convert_waveform_dict(fs, x, dat, model, mode, **kw)

    # ---- timing and pitch of a recording without analysis and synthesis: WSOLA (world/tsm.py) -------------------------
    @_hip.serialised
    def stretch_waveform(self, fs, x, ratio, hop=None, tol=None, devices=None):
        """The recording ``x`` time-stretched by waveform-similarity overlap-add: round(ratio len(x)) samples, the
        duration x ratio at the recording's own pitch (frames on an 8 ms hop moved by up to 5 ms unless told otherwise)."""
        from .tsm import stretch_waveform_numpy
        if devices is not None:
            raise NotImplementedError("stretch_waveform(devices=...): run one WorldBatch per device instead")
        return stretch_waveform_numpy(fs, x, ratio, hop, tol)

    @_hip.serialised
    def shift_pitch_waveform(self, fs, x, ratio, hop=None, tol=None, devices=None):
        """The recording ``x`` at f0 x p / q, p / q = world.tsm.as_fraction(ratio), and its own length: stretched by p / q
        and resampled by q / p.  The formants move with f0; vocoder-free conversion (convert_waveform) on the shifted
        recording moves the envelope to the target."""
        from .tsm import shift_pitch_waveform_numpy
        if devices is not None:
            raise NotImplementedError("shift_pitch_waveform(devices=...): run one WorldBatch per device instead")
        return shift_pitch_waveform_numpy(fs, x, ratio, hop, tol)

    # ---- a new f0 contour and timing for a recording: pitch-synchronous overlap-add (world/psola.py) --------------------
    @_hip.serialised
    def modify_waveform(self, fs, x, dat, pitch=1.0, f0=None, duration=1.0, devices=None):
        """The recording ``x`` with f0 x ``pitch`` (or the per-frame target ``f0`` on dat['temporal_positions']) and
        ``duration`` x as long, by pitch-synchronous overlap-add around the periods of ``dat`` = encode(fs, x): grains are
        re-spaced, not resampled, so the formants stay in place (shift_pitch_waveform moves them with f0)."""
        from .psola import modify_waveform_numpy
        if devices is not None:
            raise NotImplementedError("modify_waveform(devices=...): run one WorldBatch per device instead")
        return modify_waveform_numpy(fs, x, dat, pitch, f0, duration)

    @_hip.serialised
    def set_pitch_waveform(self, fs, x, dat, time, value, devices=None):
        """set_pitch_contour for a recording: the contour (time [s], value [Hz], 0 = unvoiced) is interpolated onto
        dat['temporal_positions'] with the voiced rule and imposed on ``x`` at its own duration."""
        from .psola import set_pitch_waveform_numpy
        if devices is not None:
            raise NotImplementedError("set_pitch_waveform(devices=...): run one WorldBatch per device instead")
        return set_pitch_waveform_numpy(fs, x, dat, time, value)

    # ---- modification (all in place on the dict, like the reference) ------------------------------------------
    def scale_pitch(self, dat, factor):
        """world/main.py:154-162."""
        dat['f0'] *= factor
        return dat

    def set_pitch(self, dat, time, value):
        raise NotImplementedError  # world/main.py:164-165

    @_hip.serialised
    def set_pitch_contour(self, dat, time, value):
        """What the reference's set_pitch describes and leaves unimplemented (world/main.py:164-168: the values "need to
        [be] resample[d] ... at given temporal positions (which are presumably shared with the spectrogram)"): the contour
        (time [s], value [Hz], 0 = unvoiced) interpolated onto dat['temporal_positions'] with np.interp's arithmetic on
        the device (BatchEncoding.set_pitch_contour, voiced rule on: no glide between 0 Hz and a voiced knot).  Replaces
        dat['f0'] and dat['vuv'], returns dat; reference dicts and encode_batch's lazy dicts alike.  set_pitch itself
        stays the reference's NotImplementedError."""
        from .regrid import interp_contour_device, knot_lists

        tp = np.ascontiguousarray(dat['temporal_positions'], dtype=np.float64)
        if tp.ndim != 1:
            raise ValueError("set_pitch_contour: temporal_positions must be 1-D, got shape %s" % (tp.shape,))
        off, t, v = knot_lists(time, value, 1, "set_pitch_contour")
        rt = _hip.Runtime.get()
        with rt.lock, rt.on_stream():
            batch = rt.make_batch([0, 0], [0, len(tp)])
            f0_d, vuv_d = interp_contour_device(rt, batch, rt.to_device(tp), off, t, v, True)
            f0, vuv = rt.torch.stack([f0_d, vuv_d]).cpu().numpy()
        dat['f0'], dat['vuv'] = f0.copy(), vuv.copy()
        return dat

    @_hip.serialised
    def regrid(self, dat, frame_period):
        """dat on the frame grid of ``frame_period`` ms (BatchEncoding.regrid for one dict): replaces temporal_positions,
        f0, vuv, spectrogram and aperiodicity — every row np.interp over the dict's own frame times, bit for bit, f0 / vuv
        by the both-bracketing rule — and returns dat.  Any source grid: another period, or the non-uniform times
        scale_duration / modify_duration leave.  Other keys ('ps spectrogram', 'coarse_ap', 'out') are left as they are."""
        from .batch import BatchEncoding, WorldBatch

        _hip.same_frames("regrid", temporal_positions=dat['temporal_positions'], f0=dat['f0'], vuv=dat['vuv'])
        wb = WorldBatch()
        new = BatchEncoding.from_dicts(wb.rt, [dat]).regrid(frame_period).to_dicts()[0]
        for key in ('temporal_positions', 'f0', 'vuv', 'spectrogram', 'aperiodicity'):
            dat[key] = new[key]
        return dat

    def scale_duration(self, dat, factor):
        """world/main.py:170-178."""
        dat['temporal_positions'] *= factor
        return dat

    def modify_duration(self, dat, from_time, to_time):
        """Piecewise-linear time map anchored at 0 and at the last frame; returns None (world/main.py:180-189)."""
        tp = dat['temporal_positions']
        last = tp[-1]
        # the reference's checks, written as it writes them (np.all(...) > 0, i.e. "not all steps are zero")
        for axis in (from_time, to_time):
            assert np.all(np.diff(axis)) > 0
        assert from_time[0] > 0 and from_time[-1] < last
        if to_time[-1] == -1:
            to_time[-1] = last
        dat['temporal_positions'] = np.interp(tp, np.r_[0, from_time, last], to_time)

    def warp_spectrum(self, dat, factor):
        """Frequency warping of every frame by f -> f**factor on the normalised axis (world/main.py:191-196)."""
        spec = dat['spectrogram']
        axis = np.arange(spec.shape[0]) / spec.shape[0]
        warped = np.stack([np.interp(axis ** factor, axis, column) for column in spec.T], axis=1)
        spec[:] = warped
        return dat

    # ---- spectral feature heads (world/main.py:257-365; world/features.py) ----------------------------------------
    def hz2mel(self, hz):
        return _feat.hz2mel(hz)

    def mel2hz(self, mel):
        return _feat.mel2hz(mel)

    def get_filterbanks(self, nfilt=20, nfft=512, samplerate=16000, lowfreq=0, highfreq=None):
        return _feat.get_filterbanks(nfilt, nfft, samplerate, lowfreq, highfreq)

    def encode_lfbank(self, spec, prefac=0.97, fs=16000, nfilt=32, lowfreq=0, highfreq=None):
        return _feat.encode_lfbank(spec, prefac, fs, nfilt, lowfreq, highfreq)

    def encode_mcep(self, spec, n0=12, fs=16000, lowhz=0, highhz=8000):
        return _feat.encode_mcep(spec, n0, fs, lowhz, highhz)

    def decode_mcep(self, cepstrum, fft_size):
        return _feat.decode_mcep(cepstrum, fft_size)

    def get_context(self, X, w=5):
        return _feat.get_context(X, w)

    # ---- mel-cepstra with an all-pass warp, the SPTK convention (world/melcep.py; no counterpart in the reference) ---
    def encode_melcep(self, spec, order=24, alpha=None, fs=16000):
        """(N, D) POWER spectrogram (encode()'s 'spectrogram', transposed) -> (N, order + 1) mel-cepstra c[0 .. order] on
        the all-pass warped axis: log P = 2 sum_j c[j] cos(j beta).  ``alpha`` None: the customary one of ``fs``
        (world.melcep.DEFAULT_ALPHA: 0.42 at 16 kHz, 0.554 at 48 kHz).  Valid at every sampling rate."""
        from . import melcep as _mc
        return _mc.encode_melcep(spec, order, alpha, fs)

    def decode_melcep(self, mc, fft_size, alpha=None, fs=16000):
        """(N, m + 1) rows of encode_melcep -> the (N, fft_size / 2 + 1) POWER spectrogram they code."""
        from . import melcep as _mc
        return _mc.decode_melcep(mc, fft_size, alpha, fs)

    def melcep_distortion(self, mc_a, mc_b):
        """(N, m + 1) rows against (N, m + 1) rows -> (N,) mel-cepstral distortion in dB,
        (10 / ln 10) sqrt(2 sum_{j >= 1} (a[j] - b[j])^2): the published MCD."""
        from . import melcep as _mc
        return _mc.melcep_distortion(mc_a, mc_b)

    def filter_waveform_melcep(self, fs, x, mc_num, mc_den=None, alpha=None, frame_period=5.0, fft_size=None):
        """The recording ``x`` filtered frame by frame by the envelope of mc_num over that of mc_den (rows of
        encode_melcep on x's frame grid; mc_den None: by mc_num's alone), in closed form: neither envelope is formed."""
        from . import melcep as _mc
        return _mc.filter_waveform_melcep(fs, x, mc_num, mc_den, alpha, frame_period, fft_size)

    # ---- line spectral frequencies (world/lsf.py; no counterpart in the reference's library) -----------------------
    def encode_lsf(self, spec, order=24):
        """(N, D) power spectrogram (encode()'s 'spectrogram', transposed) -> (N, order + 1) rows [log E, w_1 .. w_p]:
        the log of the all-pole gain and the line spectral frequencies in radians, ascending.  ``order`` even, 2 .. 64;
        valid at every sampling rate."""
        from . import lsf as _lsf
        return _lsf.encode_lsf(spec, order)

    def decode_lsf(self, lsf, fft_size, min_gap=0.0):
        """(N, p + 1) rows of encode_lsf -> the (N, fft_size / 2 + 1) all-pole power spectrogram.  ``min_gap`` > 0
        (radians) first repairs rows that are out of order or closer than that (world/lsf.py)."""
        from . import lsf as _lsf
        return _lsf.decode_lsf(lsf, fft_size, min_gap)

    def lsf_distortion(self, lsf_a, lsf_b, fft_size, gain=True, devices=None):
        """(N, p + 1) rows of encode_lsf against (N, p + 1) rows -> (N,) the log-spectral distortion in dB of the two
        all-pole envelopes on fft_size / 2 + 1 bins, frame by frame, computed from the rows without either envelope
        (world.lsf.distortion_device).  ``gain=False`` leaves the best constant gain out: the spectral shape alone."""
        from . import lsf as _lsf
        if devices is not None:
            raise NotImplementedError("lsf_distortion(devices=...): run one WorldBatch per device instead")
        return _lsf.lsf_distortion(lsf_a, lsf_b, fft_size, gain)

    def encode_lpc(self, spec, order=24):
        """(N, D) power spectrogram -> (a (N, order + 1) with a[:, 0] = 1, the prediction-error gain E (N,), the
        reflection coefficients (N, order))."""
        from . import lsf as _lsf
        return _lsf.encode_lpc(spec, order)

    # ---- manifold vocoder (world/main.py:367-384; world/manifold.py) ----------------------------------------------
    def encode_vae(self, Xc, energy, encoder, decoder, window, n0, batch_size, mean):
        """MCEP -> latent -> MCEP through the VAE's encoder and decoder (world/main.py:367-384), both networks in one
        device launch, FP64 throughout (the reference's Keras runs float32: results differ by float32 rounding).

        ``Xc``: (N, n0-1) MCEP without the energy column; ``energy``: (N,) column 0.  ``encoder`` / ``decoder``: each a
        world.manifold.DenseStack, a Keras-like model or the path of a Keras HDF5 file.  ``batch_size`` is accepted and
        ignored (the whole input is one launch).  As in the reference, ``Xc -= mean`` mutates the caller's array.
        Returns (Zc, Yc): the latent as float32 (Keras predict's dtype) and (N, n0) float64 MCEP with ``energy`` in
        column 0.  The latent goes on to the decoder rounded to float32, as between Keras' two predict calls."""
        assert Xc.shape[1] == n0 - 1
        x = np.array(Xc, dtype=np.float64)  # the kernel subtracts the mean itself, with the same rounding
        args = _vae_args(x, energy, n0, mean, window)
        Xc -= mean
        return self._vae(x, *args, encoder=encoder, decoder=decoder)

    def decode_vae(self, Zc, energy, decoder, window, n0, mean):
        """Extension (not in the reference): the decoder half of encode_vae on a latent ``Zc`` (N, latent), e.g. one
        edited for a conversion.  Returns Yc (N, n0) as encode_vae does; decode_vae(encode_vae(...)[0], ...) gives
        encode_vae's Yc bit for bit."""
        z = np.asarray(Zc)
        return self._vae(z, *_vae_args(z, energy, n0, mean, window), decoder=decoder)[1]

    @_hip.serialised
    def _vae(self, x, energy, n0, m, window, encoder=None, decoder=None):
        n = x.shape[0]
        dec = _man.as_stack(decoder)
        enc = _man.as_stack(encoder) if encoder is not None else None
        zc = np.zeros((n, enc.units[-1] if enc is not None else x.shape[1]), dtype=np.float32)
        yc = np.zeros((n, n0))
        yc[:, 0] = energy
        if n:
            rt = _hip.Runtime.get()
            x_d = rt.to_device(np.ascontiguousarray(x, dtype=np.float64))
            if enc is not None:
                z_d, y_d = _man.vae_device(rt, x_d, enc, dec, window, m)
                zc = z_d.cpu().numpy().astype(np.float32)
            else:
                y_d = _man.decode_vae_device(rt, x_d, dec, n0 - 1, window, m)
            yc[:, 1:] = y_d.cpu().numpy()
        return zc, yc

    # ---- synthesis ----------------------------------------------------------------------------------------------
    def decode(self, dat):
        """world/main.py:198-214: pulse-wise or Requiem synthesis, then peak normalisation above 1."""
        _check_decodable([dat])
        if dat['is_requiem']:
            y = _synr.synthesisRequiem(dat, dat, _seeds.get_seeds_signals(dat['fs']))
        else:
            y = _syn.synthesis(dat, dat)
        peak = np.max(np.abs(y))
        if peak > 1.0:
            logging.info('rescaling waveform')
            y /= peak
        dat['out'] = y
        return dat
