"""GPU: the minimum-phase chain with the table-driven exponentials (csrc/wh_minphase.h: cis_pair_call on wh_math.h's texp /
tsincospi) against the oracle's decode, at the smallest inputs at which the chain can still go wrong: 20 frames at each
of the three transform lengths with a path of their own (N = 512 at 8 kHz, N = 1024 at 16 kHz: the wave-local chains,
N = 2048 at 48 kHz: 512 threads per pulse), a voiced stretch, an unvoiced stretch and the boundary between them; spectrogram
rows from exact zeros (the eps substitution in front of the logarithm) over 1e-16 to 1e6, so that the exponentials'
arguments span their range; pitch periods of a whole number of samples (every pulse's fractional delay next to 0 or next
to 1) and of a whole number and a half.  Host noise: the comparison is sample-exact in structure.  The tolerance is the
decode's (tests/test_hip_synthesis.py): relative RMS < 1e-9."""
import numpy as np
import pytest

from conftest import rel_rms

pytestmark = pytest.mark.gpu

FRAMES = 20


def _encoding(fs, seed):
    rng = np.random.RandomState(seed)
    n = {8000: 512, 16000: 1024, 48000: 2048}[fs]
    k = n // 2 + 1
    tp = np.arange(FRAMES) * 0.005
    vuv = np.zeros(FRAMES)
    vuv[:11] = 1.0
    f0 = np.zeros(FRAMES)
    f0[:6] = fs / 100.0    # period 100 samples: the pulses fall on (or a rounding error beside) whole samples
    f0[6:11] = fs / 90.5   # period 90.5 samples: fractional delays of 0 and 1/2 alternate, drifting through the change
    # rows between 1e-16 and 1e6, smooth along the bins on one half of the frames and bin-to-bin random on the other
    smooth = 10.0 ** (-5.0 + 11.0 * np.cos(np.linspace(0, 5 * np.pi, k))[:, None] * np.ones((1, FRAMES)))
    rough = 10.0 ** rng.uniform(-16, 6, (k, FRAMES))
    spec = np.where(np.arange(FRAMES)[None, :] % 2 == 0, smooth, rough)
    spec[[0, 7, k // 2, k - 1], :] = rng.uniform(0.5, 2.0, (4, FRAMES))  # (around 1: log amplitudes next to 0)
    spec[[3, k // 3, k - 2], :] = 0.0                                      # exact zeros in every frame: eps is substituted
    ap = rng.uniform(0.01, 0.99, (k, FRAMES))
    ap[:, vuv == 0] = 1 - 1e-12
    ap[:, 9] = 1 - 1e-12  # a voiced frame whose aperiodicity says noise only (the pulse takes the unvoiced path)
    return {"f0": f0, "vuv": vuv, "temporal_positions": tp, "spectrogram": spec, "aperiodicity": ap, "fs": fs,
            "is_requiem": False}


_cases = {}


def _case(fs):
    """(encoding, noise, the oracle's decode), computed once per rate"""
    if fs not in _cases:
        from oracle import api as oapi

        dat = _encoding(fs, fs // 1000)
        noise = np.random.RandomState(fs // 1000 + 100).randn(8 * int(0.005 * FRAMES * fs) + 4096)
        ref = oapi.decode_np(dict(dat), noise=noise)["out"]
        ref.setflags(write=False)
        _cases[fs] = (dat, noise, ref)
    return _cases[fs]


@pytest.mark.parametrize("fs", [16000, 8000, 48000])
def test_decode_matches_the_oracle(fs):
    from world.batch import BatchEncoding, WorldBatch

    dat, noise, ref = _case(fs)
    wb = WorldBatch()
    enc = BatchEncoding.from_dicts(wb.rt, [dat])
    assert enc.fft_size == {8000: 512, 16000: 1024, 48000: 2048}[fs]
    y, off = wb.decode_device(enc, noise=[noise])
    y = y.cpu().numpy()[off[0]:off[1]]
    assert len(y) == len(ref)
    assert np.all(np.isfinite(y)) and np.max(np.abs(ref)) > 0
    err = rel_rms(y, ref)
    print("fs %d: relative RMS against the oracle %.3g" % (fs, err))
    assert err < 1e-9
    assert wb.rt.take_flags() == [0] * 16


def test_two_utterances_in_one_batch_are_the_solo_decodes():
    """The pair path of response_kernel<1024> (two unvoiced pulses side by side) and the runs of a batch read the same tables:
    a batch of the case and its copy decodes to the solo result twice, bit for bit."""
    from world.batch import BatchEncoding, WorldBatch

    dat, noise, ref = _case(16000)
    wb = WorldBatch()
    y1, off1 = wb.decode_device(BatchEncoding.from_dicts(wb.rt, [dat]), noise=[noise])
    y2, off2 = wb.decode_device(BatchEncoding.from_dicts(wb.rt, [dat, dict(dat)]), noise=[noise, noise])
    y1, y2 = y1.cpu().numpy(), y2.cpu().numpy()
    assert np.array_equal(y2[off2[0]:off2[1]], y1) and np.array_equal(y2[off2[1]:off2[2]], y1)
