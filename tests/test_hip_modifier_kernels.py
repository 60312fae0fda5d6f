"""GPU: the kernels of csrc/wh_modify.hip on their own — warp_spectrum_kernel at every frame length up to the largest the
C-ABI accepts (16385 bins: the branch with more than 64 KiB of dynamic LDS), whole frames against np.interp bit for bit;
modify_duration_kernel with anchor tables that differ per utterance; the two PCM conversions over their whole domain.
Non-finite spectra are left to tests/test_hip_nonfinite.py (np.interp has a NaN fallback the kernel does not claim)."""
import ctypes

import numpy as np
import pytest

from test_feature_tables_host import WARP_FACTORS, WARP_K, bits, pcm_inputs, ref_pcm16, ref_warp, warp_frames

pytestmark = pytest.mark.gpu

_vp = ctypes.c_void_p


def _rt():
    from world import _hip

    return _hip.Runtime.get()


def _warp_rc(rt, spec_d, k_bins, factor):
    """wh_warp_spectrum on a frame-major [F][k_bins] device tensor, in place; the return code."""
    from world._tables import warp_tables

    src, dx, den = warp_tables(int(k_bins), float(factor))
    return rt.lib.wh_warp_spectrum(rt.ctx, rt.stream(), rt.ptr(spec_d), int(spec_d.shape[0]), int(k_bins),
                                   src.ctypes.data_as(_vp), dx.ctypes.data_as(_vp), den.ctypes.data_as(_vp))


# ---- a. wh_warp_spectrum -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k_bins", WARP_K)
def test_warp_spectrum_equals_interp_bit_for_bit(k_bins):
    """K = 16385 needs 131 080 B of LDS (wh::allow_lds); 4097 is the largest of the list below 64 KiB."""
    from world import _hip

    rt = _rt()
    frames = warp_frames(5, k_bins, 3 * k_bins)
    assert np.all(np.isfinite(frames)) and np.sum(frames == 0) == 1 and np.sum(frames == 5e-324) == 1
    frames_d = rt.to_device(frames)
    for factor in WARP_FACTORS:
        work = frames_d.clone()
        _hip.check(_warp_rc(rt, work, k_bins, factor))
        got, ref = work.cpu().numpy(), ref_warp(frames, factor)
        bad = np.argwhere(bits(got) != bits(ref))
        assert len(bad) == 0, "K %d factor %r: %d bins differ, the first in frame %d bin %d: %r for %r" % (
            k_bins, factor, len(bad), bad[0][0], bad[0][1], got[tuple(bad[0])], ref[tuple(bad[0])])
    assert np.array_equal(bits(frames_d.cpu().numpy()), bits(frames))


@pytest.mark.parametrize("k_bins", WARP_K)
def test_warp_spectrum_300_frames(k_bins):
    """More workgroups than the chip has compute units once K is large (one frame each, up to 128 KiB of LDS)."""
    from world import _hip

    rt = _rt()
    frames = warp_frames(300, k_bins, 5 * k_bins)
    work = rt.to_device(frames)
    _hip.check(_warp_rc(rt, work, k_bins, 1.1))
    assert np.array_equal(bits(work.cpu().numpy()), bits(ref_warp(frames, 1.1)))


@pytest.mark.parametrize("k_bins", (1, 16386))
def test_warp_spectrum_refuses_a_frame_length_out_of_range(k_bins):
    rt = _rt()
    frames = warp_frames(2, max(k_bins, 2), 1)[:, :k_bins].copy()
    work = rt.to_device(frames)
    assert _warp_rc(rt, work, k_bins, 1.1) != 0
    assert b"k_bins out of range" in rt.lib.wh_last_error()
    assert np.array_equal(bits(work.cpu().numpy()), bits(frames))


# ---- b. BatchEncoding.modify_duration ------------------------------------------------------------------------------------------
FRAMES = (141, 203, 317)  # last frame times 0.7, 1.01, 1.58 s
# interior anchors; in the last set 0.125, 0.25, 0.5 and 0.625 are frame times (multiples of 5 ms that are exact in binary)
ANCHORS = ([0.3], [0.25, 0.5], [0.05, 0.125, 0.25, 0.3, 0.5, 0.55, 0.625])


def _encoding(rt):
    from world.batch import BatchEncoding

    dats = []
    for u, nf in enumerate(FRAMES):
        dats.append({"f0": np.full(nf, 100.0 + u), "vuv": np.ones(nf), "temporal_positions": np.arange(0, nf) * 5 / 1000,
                     "spectrogram": np.ones((3, nf)), "aperiodicity": np.full((3, nf), 0.5), "fs": 16000,
                     "is_requiem": False})
    return BatchEncoding.from_dicts(rt, dats), [d["temporal_positions"] for d in dats]


@pytest.mark.parametrize("trailing", ("end", "explicit"))
@pytest.mark.parametrize("scale", (0.5, 1.1), ids=("compress", "stretch"))
@pytest.mark.parametrize("anchors", ANCHORS, ids=lambda a: "%d-anchors" % len(a))
def test_modify_duration_per_utterance(anchors, scale, trailing):
    rt = _rt()
    enc, tps = _encoding(rt)
    for f in (25, 50, 100, 125):
        assert tps[0][f] in ANCHORS[2]  # the frame times the 7-anchor set sits on: np.interp's xp[j] == x branch
    # a monotone map that is not linear: every other anchor is pulled back a little
    to_time = [0.0] + [scale * t * (0.95 if i % 2 else 1.0) for i, t in enumerate(anchors)] + [-1 if trailing == "end" else 3.0]
    before = enc.temporal_positions
    before_bits = bits(before.cpu().numpy())
    assert enc.modify_duration(list(anchors), list(to_time)) is enc
    after = enc.temporal_positions
    assert after is not before and after.data_ptr() != before.data_ptr()  # a NEW array, like the reference installs
    assert np.array_equal(bits(before.cpu().numpy()), before_bits)
    got = after.cpu().numpy()
    fo = enc.batch.frame_off
    for u, tp in enumerate(tps):
        end = tp[-1]
        fp = list(to_time)
        if fp[-1] == -1:
            fp[-1] = end
        ref = np.interp(tp, np.r_[0, anchors, end], fp)  # world/main.py:180-189, this utterance's own `end`
        assert np.array_equal(bits(got[int(fo[u]):int(fo[u + 1])]), bits(ref)), (u, len(anchors), scale, trailing)
    assert np.array_equal(enc.host_times(), got)


# ---- c. PCM --------------------------------------------------------------------------------------------------------------------
PCM_LENGTHS = (1, 255, 256, 257, 65537)
TAIL = 64


def _to_f64(rt, pcm):
    from world import _hip

    n = len(pcm)
    out = rt.torch.full((n + TAIL,), -7.0, dtype=rt.torch.float64, device=rt.device)
    pcm_d = rt.torch.from_numpy(np.ascontiguousarray(pcm, dtype=np.int16)).to(rt.device)
    _hip.check(rt.lib.wh_pcm16_to_f64(rt.ctx, rt.stream(), rt.ptr(pcm_d), n, rt.ptr(out)))
    out = out.cpu().numpy()
    assert np.all(out[n:] == -7.0)
    return out[:n]


def _to_pcm16(rt, y):
    from world import _hip

    n = len(y)
    out = rt.torch.full((n + TAIL,), 12345, dtype=rt.torch.int16, device=rt.device)
    _hip.check(rt.lib.wh_f64_to_pcm16(rt.ctx, rt.stream(), rt.ptr(rt.to_device(y)), n, rt.ptr(out)))
    out = out.cpu().numpy()
    assert np.all(out[n:] == 12345)
    return out[:n]


def test_pcm16_to_f64_over_every_value():
    rt = _rt()
    every = np.arange(-32768, 32768).astype(np.int16)
    assert len(np.unique(every)) == 65536
    assert np.array_equal(bits(_to_f64(rt, every)), bits(every / 32767.0))  # example/prosody.py:13
    for n in PCM_LENGTHS:
        pcm = np.resize(every[::-7], n)
        assert np.array_equal(bits(_to_f64(rt, pcm)), bits(pcm / 32767.0)), n


@pytest.mark.parametrize("n", PCM_LENGTHS + (None,))
def test_f64_to_pcm16_against_the_integer_restatement(n):
    rt = _rt()
    y = pcm_inputs()
    if n is not None:
        y = np.resize(y[::-1], n)  # (reversed: the short lengths hold the listed, the non-finite and the edge values)
    got, ref = _to_pcm16(rt, y), ref_pcm16(y)
    bad = np.flatnonzero(got != ref)
    assert len(bad) == 0, "%d differ, the first: %r -> %d, restatement %d" % (len(bad), y[bad[0]], got[bad[0]], ref[bad[0]])
