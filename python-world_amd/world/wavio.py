"""Batched 16-bit WAV input / output around the resident pipeline, with the reference callers'
conventions (example/prosody.py:12-13,57; test/speed.py:14): x = int16 / (2**15 - 1) on the way in,
(out * 2**15).astype(int16) on the way out.  The conversions run on the device (wh_pcm16_to_f64 / wh_f64_to_pcm16), so
only 2-byte samples cross PCIe.  Corpora at mixed rates are resampled on the device (``resample_to`` / ``out_fs``:
scipy.signal.resample_poly bit for bit, world.resample)."""
import numpy as np


def _read_one(p):
    from scipy.io import wavfile

    fs, x = wavfile.read(str(p))
    if x.ndim != 1 or x.dtype != np.int16:
        raise ValueError("%s: expected 16-bit mono PCM" % p)
    return int(fs), x


def read_wavs(paths):
    """(fs, [int16 mono arrays]) of a list of WAV files that share one sampling rate."""
    fs0, out = None, []
    for p in paths:
        fs, x = _read_one(p)
        if fs0 is not None and fs != fs0:
            raise ValueError("%s: sampling rate %d differs from %d" % (p, fs, fs0))
        fs0 = fs
        out.append(x)
    return fs0, out


def encode_wavs(paths, world_batch=None, resample_to=None, **encode_kw):
    """Read, upload as int16 and encode a list of WAV files: (fs, BatchEncoding).  ``resample_to``: a rate; the files
    may then have mixed rates, each is resampled to it on the device (resample_poly(x, resample_to, fs) of the scaled
    samples, example/prosody.py:16-19) and the result is (resample_to, BatchEncoding)."""
    from .batch import WorldBatch

    wb = world_batch or WorldBatch()
    if resample_to is not None:
        read = [_read_one(p) for p in paths]
        batch, x_d, tp_d = wb.upload_resampled([x for _, x in read], [fs for fs, _ in read], int(resample_to),
                                               encode_kw.get("frame_period", 5))
        return int(resample_to), wb.encode_device(batch, x_d, tp_d, int(resample_to), **encode_kw)
    fs, pcm = read_wavs(paths)
    batch, x_d, tp_d = wb.upload_pcm16(pcm, fs, encode_kw.get("frame_period", 5))
    return fs, wb.encode_device(batch, x_d, tp_d, fs, **encode_kw)


def write_wavs(paths, fs, world_batch, y, y_off, out_fs=None):
    """Write decode_device's output as one 16-bit WAV per utterance.  ``out_fs``: resample the audio from ``fs`` to this
    rate on the device (WorldBatch.resample_device) before the PCM conversion, and write the files at it."""
    from scipy.io import wavfile

    if out_fs is not None and int(out_fs) != int(fs):
        y, y_off = world_batch.resample_device(y, y_off, int(fs), int(out_fs))
        fs = int(out_fs)
    pcm = world_batch.to_pcm16(y, y_off)
    if len(pcm) != len(paths):
        raise ValueError("%d paths for %d utterances" % (len(paths), len(pcm)))
    for p, v in zip(paths, pcm):
        wavfile.write(str(p), int(fs), v)
