"""response_kernel's pairs: at the 16 kHz shape two consecutive unvoiced pulses of a run (both records say vuv == 0, the
noise is the device stream's, both noise runs fit the 256-sample buffer together) go through the two chain buffers side
by side, like the two chains of a voiced pulse; every other pulse goes alone.  The contours below are hand-built so that
every way into and out of a pair occurs; `_plan` restates the kernel's rule on the oracle's pulse list, and the CPU test
asserts from it that each situation is really there."""
import numpy as np
import pytest

from conftest import rel_rms

FS = 16000
NFFT = 1024
K = NFFT // 2 + 1
HOP = 0.005
SEED = 77012
RUN = 6    # pulses per workgroup at this transform length
NZ = 256   # samples of the kernel's noise buffer


def _envelope(rng, frames):
    """A smooth positive spectrogram (bins, frames) that differs from frame to frame."""
    k = np.arange(K)[:, None] / K
    sp = 1e-3 * np.exp(-4.0 * k) * (1.0 + 0.5 * np.sin(0.7 * np.arange(frames))[None, :])
    for _ in range(4):
        c = rng.uniform(0.02, 0.6, size=(1, frames)).cumsum(axis=1) / np.arange(1, frames + 1)
        sp = sp + rng.uniform(1e-4, 2e-3) * np.exp(-0.5 * ((k - c) / 0.03) ** 2)
    return sp


def _dat(f0, vuv, sp, ap):
    frames = len(f0)
    vuv = np.asarray(vuv, dtype=np.float64)
    return {"temporal_positions": np.arange(frames) * HOP, "vuv": vuv, "fs": FS,
            "f0": np.asarray(f0, dtype=np.float64) * vuv, "aperiodicity": ap, "spectrogram": sp, "is_requiem": False}


def _ap(rng, frames):
    return np.clip(0.2 + 0.6 * np.arange(K)[:, None] / K + 0.05 * rng.rand(K, frames), 0.0, 0.98)


def _plan(d):
    """The oracle's pulse list with what the kernel decides from it: per pulse the 1-based index, noise_size, stream offset,
    vuv at the pulse, voiced (vuv and aperiodicity[0] <= 0.999), the pair of frames it interpolates; `first` / `second`:
    the pulse is the first / second of a pair under device noise (runs of RUN pulses, walked in order: two pulses pair when
    both have vuv == 0 and max(3, size) of both together is at most NZ)."""
    from oracle import common as C
    from oracle import resynth

    tp = d["temporal_positions"]
    times, idx, _, vuv_i, t = resynth.pulse_train(tp, d["f0"], FS, d["vuv"])
    n = len(idx)
    size = idx[np.minimum(n - 1, np.arange(n) + 1)] - idx
    nd = np.maximum(3, size)
    off = np.concatenate([[0], np.cumsum(nd)])
    pos = np.maximum(1, np.minimum(len(tp), C.lerp_extrap(tp, np.arange(1, len(tp) + 1, dtype=np.float64), times)))
    lo, hi = np.floor(pos).astype(np.int64) - 1, np.ceil(pos).astype(np.int64) - 1
    same = tp[lo] == tp[hi]
    b = np.where(same, 0.0, (np.clip(times, tp[lo], tp[hi]) - tp[lo]) / np.where(same, 1.0, tp[hi] - tp[lo]))
    ap2 = d["aperiodicity"][0] ** 2
    aper0 = np.where(same, ap2[lo], (1 - b) * ap2[lo] + b * ap2[hi])
    vuv0 = vuv_i[idx - 1]
    voiced = vuv0 & (aper0 <= 0.999)
    first, second = np.zeros(n, bool), np.zeros(n, bool)
    rejected_by_size = np.zeros(n, bool)  # both vuv == 0, in one run, but the two runs do not fit the buffer
    for r0 in range(0, n, RUN):
        i, r1 = r0, min(n, r0 + RUN)
        while i < r1:
            if i + 1 < r1 and not vuv0[i] and not vuv0[i + 1]:
                if nd[i] + nd[i + 1] <= NZ:
                    first[i], second[i + 1] = True, True
                    i += 2
                    continue
                rejected_by_size[i] = True
            i += 1
    return {"idx": idx, "size": size, "nd": nd, "off": off, "ny": len(t), "vuv0": vuv0, "voiced": voiced, "lo": lo, "hi": hi,
            "first": first, "second": second, "rejected_by_size": rejected_by_size, "slot": np.arange(n) % RUN}


def _unvoiced(rng, want_odd_tail):
    """An utterance without a voiced frame (pulses every 2 ms) whose last run holds an odd / an even number of pulses."""
    for frames in range(44, 80):
        f0 = np.zeros(frames)
        d = _dat(f0, f0, _envelope(np.random.RandomState(frames), frames), _ap(np.random.RandomState(frames + 1), frames))
        tail = len(_plan(d)["idx"]) % RUN
        if (tail % 2 == 1) == want_odd_tail and tail != 0:
            return d
    raise AssertionError("no such length")


def _batch():
    rng = np.random.RandomState(11)
    dats = [_unvoiced(rng, False), _unvoiced(rng, True)]
    # 2: an unvoiced utterance with single voiced frames at irregular distances (one voiced pulse, or a few, between
    # unvoiced ones: pairs start at odd and at even slots), a stretch of voiced frames whose aperiodicity is 1 (vuv != 0,
    # unvoiced by the rows only), and a voiced end at 40 Hz: the contour climbs from 0 there, so the last unvoiced pulse
    # in front of it has a noise run of several hundred samples
    # (the onset of that end is moved frame by frame until the long run is the SECOND of two vuv == 0 pulses of one run)
    frames = 150
    ap = _ap(rng, frames)
    ap[:, 78:102] = 1.0
    sp = _envelope(rng, frames)
    for onset in range(116, 130):
        f0 = np.zeros(frames)
        for at in (7, 18, 27, 39, 46, 58, 65):
            f0[at] = 170.0
        f0[80:100] = 400.0
        f0[onset:] = 40.0
        d = _dat(np.where(f0 > 0, f0, 1.0), (f0 > 0).astype(np.float64), sp, ap)
        if _plan(d)["rejected_by_size"].any():
            break
    dats.append(d)
    # 3: flat spectrum 1/64 without a voiced frame: every response is an impulse of height 1/8 at the pulse's own sample,
    # the runs do not overlap, and the output IS the zero-mean noise
    frames = 61
    dats.append(_dat(np.zeros(frames), np.zeros(frames), np.full((K, frames), 1.0 / 64), np.full((K, frames), 0.5)))
    return dats


def test_contours_have_every_way_into_and_out_of_a_pair():
    """(no GPU) each situation the GPU test relies on occurs in its input."""
    dats = _batch()
    plans = [_plan(d) for d in dats]
    p0, p1, p2, p3 = plans
    # long unvoiced stretches: every full run is three pairs; the last run of utterance 0 is even, of utterance 1 odd
    for p in (p0, p1, p3):
        assert not p["vuv0"].any() and len(p["idx"]) >= 8 * RUN and (p["nd"] <= 40).all()
    n0, n1 = len(p0["idx"]), len(p1["idx"])
    assert n0 % RUN in (2, 4) and p0["first"].sum() * 2 == n0
    assert n1 % RUN in (1, 3, 5) and p1["first"].sum() * 2 == n1 - 1
    # an unvoiced pulse that is the last of its utterance and of a run, and goes alone
    assert not p1["first"][-1] and not p1["second"][-1] and not p1["vuv0"][-1]
    # a single voiced pulse between unvoiced ones; pairs that start at odd slots
    v = p2["voiced"]
    assert ((~p2["vuv0"][:-2]) & v[1:-1] & (~p2["vuv0"][2:])).any()
    assert (p2["first"] & (p2["slot"] % 2 == 1)).any() and (p2["first"] & (p2["slot"] % 2 == 0)).any()
    assert (~p2["vuv0"] & ~p2["first"] & ~p2["second"]).any()  # an unvoiced pulse left over inside a run
    # pairs that interpolate one pair of frames, and pairs that straddle a frame boundary
    for p in plans:
        f = np.nonzero(p["first"])[0]
        same_rows = (p["lo"][f] == p["lo"][f + 1]) & (p["hi"][f] == p["hi"][f + 1])
        assert same_rows.any() and (~same_rows).any()
    # vuv != 0 and aperiodicity[0] > 0.999: unvoiced by the rows only, never in a pair
    rows_only = p2["vuv0"] & ~p2["voiced"]
    assert rows_only.sum() >= 10 and not (rows_only & (p2["first"] | p2["second"])).any()
    # two vuv == 0 pulses of one run whose noise runs do not fit the buffer together
    assert p2["rejected_by_size"].any()
    assert ((p2["nd"] > NZ) & ~p2["vuv0"]).any()  # (and one whose own run does not fit: the chunked path)
    # voiced pulses with two chains are there as well
    assert p2["voiced"].sum() >= 10


def test_flat_spectrum_output_is_the_noise_on_the_oracle():
    """(no GPU) what the Philox check relies on, shown on the oracle: utterance 3 decodes to (run - its mean) / 8."""
    from oracle import api as oapi

    d = _batch()[3]
    p = _plan(d)
    z = np.random.RandomState(1).randn(int(p["off"][-1]))
    y = oapi.decode_np(dict(d), noise=z)["out"]
    assert np.max(np.abs(y)) < 1.0  # (not peak-normalised)
    for i in range(len(p["idx"]) - 1):
        run = z[p["off"][i]:p["off"][i + 1]]
        assert np.max(np.abs(y[p["idx"][i]:p["idx"][i] + p["nd"][i]] - (run - run.mean()) / 8)) < 1e-12, i


@pytest.mark.gpu
def test_pairs_decode_matches_oracle_streams_and_is_repeatable():
    """(a) the seeded decode against the oracle fed the dumped device stream, at test_hip_response_roles.py's tolerance
    (1e-9 relative RMS, 1e-9 x max(scale, 1) absolute), utterance by utterance: even and odd runs, voiced pulses between
    pairs, pairs across a frame boundary, pulses unvoiced by the rows only, runs too long to pair;
    (b) the same with host-supplied noise (the dumped stream): never paired, the same tolerance;
    (c) the normals a paired pulse consumes are wh_philox_normals' for the same seed / utterance / offset: utterance 3's
    output is (run - mean) / 8 at every pulse, compared at 1e-12 (a run shifted by one sample, or two runs swapped, is off
    by O(0.1); the arithmetic may differ by the order of the mean's sum and the rounding of three transforms of a
    constant, ~1e-14);
    (d) two seeded decodes are bitwise equal, and every utterance decoded at the same batch position among other
    neighbours equals its row of the batch."""
    from oracle import api as oapi
    from world.batch import BatchEncoding, WorldBatch
    from world.synthesis import philox_normals

    dats = _batch()
    plans = [_plan(d) for d in dats]
    assert all(p["first"].any() for p in plans) and plans[2]["rejected_by_size"].any()
    wb = WorldBatch()
    enc = BatchEncoding.from_dicts(wb.rt, dats)
    y, off = wb.decode_device(enc, seed=SEED)
    y = y.cpu().numpy()
    assert wb.rt.take_flags() == [0] * 16
    dump = [philox_normals(wb.rt, SEED, u, int(p["off"][-1]) + 64).cpu().numpy() for u, p in enumerate(plans)]
    scale = np.max(np.abs(y))
    assert scale > 1e-3
    # (a)
    ref = []
    for u, d in enumerate(dats):
        yo = oapi.decode_np(dict(d), noise=dump[u])["out"]
        ref.append(yo)
        seg = y[off[u]:off[u + 1]]
        assert len(seg) == len(yo) == plans[u]["ny"]
        rr, ma = rel_rms(seg, yo), np.max(np.abs(seg - yo))
        print("seeded, utterance %d: rel rms %.3e, max abs %.3e (scale %.3e)" % (u, rr, ma, scale))
        assert rr < 1e-9
        assert ma < 1e-9 * max(scale, 1.0)
    # (b)
    yh, offh = wb.decode_device(enc, noise=dump)
    yh = yh.cpu().numpy()
    assert wb.rt.take_flags() == [0] * 16 and np.array_equal(off, offh)
    for u in range(len(dats)):
        seg = yh[off[u]:off[u + 1]]
        rr, ma = rel_rms(seg, ref[u]), np.max(np.abs(seg - ref[u]))
        print("host noise, utterance %d: rel rms %.3e, max abs %.3e" % (u, rr, ma))
        assert rr < 1e-9
        assert ma < 1e-9 * max(scale, 1.0)
    # (c)
    p = plans[3]
    seg = y[off[3]:off[4]]
    worst, checked, paired = 0.0, 0, 0
    for i in range(len(p["idx"]) - 1):
        run = dump[3][p["off"][i]:p["off"][i + 1]]
        worst = max(worst, np.max(np.abs(seg[p["idx"][i]:p["idx"][i] + p["nd"][i]] - (run - run.mean()) / 8)))
        checked += 1
        paired += bool(p["first"][i] or p["second"][i])
    print("noise runs: %d pulses (%d in pairs), worst |out - (run - mean) / 8| %.3e" % (checked, paired, worst))
    assert checked >= 8 * RUN and paired >= checked - RUN
    assert worst < 1e-12
    # (d)
    y2, off2 = wb.decode_device(enc, seed=SEED)
    assert np.array_equal(off, off2) and np.array_equal(y2.cpu().numpy(), y)
    filler = _dat(np.full(24, 120.0), np.ones(24), dats[0]["spectrogram"][:, :24], dats[0]["aperiodicity"][:, :24])
    for u, d in enumerate(dats):
        other = WorldBatch()
        e1 = BatchEncoding.from_dicts(other.rt, [filler] * u + [d])
        y1, o1 = other.decode_device(e1, seed=SEED)
        assert np.array_equal(y1.cpu().numpy()[o1[u]:o1[u + 1]], y[off[u]:off[u + 1]]), u
