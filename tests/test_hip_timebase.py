"""GPU: the synthesis time base (csrc/wh_timebase.hip: prep_kernel, the exact phase scan, pulse_mark / scan / emit /
finish / frames) compared PULSE BY PULSE with the reference in plain NumPy (tests/_timebase_reference.py, pinned on the
CPU by tests/test_timebase_reference_host.py) through the read-back wh_synthesis_timebase_read.

No tolerance anywhere: pulse counts, 1-based indices, noise offsets and sizes, per-pulse voicing, both frame rows and the
per-sample voicing are integers; pulse time, fractional shift, frame weight and the cumulative phase are results of
IEEE-exact operations in the reference's order (fmod, subtraction, correctly rounded division, the bit-exact scan; the
unit is built with contraction off) and are compared as int64 views.  The cases (tests/_timebase_cases.py) put crossings on
the 1024-sample seam of pulse_mark_kernel and on the last pair ny - 2 / ny - 1, phase steps of exactly pi, noise sizes below
3, pulses and samples exactly on frame times, uneven and stretched frame grids, tp[0] of 0.5 and 3 samples, a negative last
increment, and one utterance long enough for the tile-parallel scan."""
import ctypes
import zlib

import numpy as np
import pytest

import _timebase_cases as TC
import _timebase_reference as TR

pytestmark = pytest.mark.gpu

_refs = {}


def fft_for(fs):
    """CheapTrick's transform length at ``fs`` (world/cheaptrick.py:24): what encode() derives the fused limit from"""
    return int(2 ** np.ceil(np.log2(3.0 * fs / 71.0 + 1)))


def fused_f0(c):
    return TR.final_f0(c.f0, c.vuv, TR.low_limit(c.fs, getattr(c, "fft_size", None) or fft_for(c.fs)))


def ref_of(c, fused=False):
    key = (c.name, bool(fused))
    if key not in _refs:
        _refs[key] = TR.timebase_np(c.tp, fused_f0(c) if fused else c.f0, c.vuv, c.fs)
    return _refs[key]


def _rt():
    from world import _hip

    return _hip.Runtime.get()


class _Batch:
    """device arrays and the time-axis geometry of a list of (tp, f0, vuv) at one rate"""

    def __init__(self, rt, utts, fs):
        from world.synthesis import time_axis_params

        self.n = len(utts)
        self.fs = fs
        nf = [len(u[0]) for u in utts]
        self.frame_off = np.concatenate([[0], np.cumsum(nf)]).astype(np.int64)
        self.batch = rt.make_batch(np.zeros(self.n + 1, dtype=np.int64), self.frame_off)
        geo = [time_axis_params(u[0], fs) for u in utts]
        self.ny = [g[0] for g in geo]
        self.t0 = [g[1] for g in geo]
        self.dt = [g[2] for g in geo]
        self.tp_d = rt.to_device(np.concatenate([u[0] for u in utts]))
        self.f0_d = rt.to_device(np.concatenate([u[1] for u in utts]))
        self.vuv_d = rt.to_device(np.concatenate([u[2] for u in utts]))


def run_timebase(utts, fs, cap, limit=0.0):
    """(per-utterance read-back, flags) of wh_synthesis_timebase on a batch of (tp, f0, vuv)"""
    from world.synthesis import synthesis_timebase_device, synthesis_timebase_read

    rt = _rt()
    rt.take_flags()
    b = _Batch(rt, utts, fs)
    synthesis_timebase_device(rt, b.batch, b.tp_d, b.f0_d, b.vuv_d, fs, b.ny, b.t0, b.dt, cap, f0_low_limit=limit)
    got = synthesis_timebase_read(rt, b.n, cap, b.ny)
    return got, rt.take_flags()


def _utt(c):
    return (c.tp, c.f0, c.vuv)


def _flags(**set_):
    from world import _hip

    f = [0] * 16
    for k, v in set_.items():
        f[getattr(_hip, "FLAG_" + k)] = v
    return f


def _raised(flags):
    return [int(bool(f)) for f in flags]


# ---- every case alone, both forms ------------------------------------------------------------------------------------

def test_read_back_needs_a_time_base():
    """fails before any time-base call of a context, and after a call that lays the workspace out again"""
    from world import _hip
    from world.synthesis import synthesis_plan, synthesis_timebase_device, synthesis_timebase_read

    rt = _rt()
    fresh = ctypes.c_void_p()
    _hip.check(rt.lib.wh_ctx_create(rt.index, ctypes.byref(fresh)))
    try:
        null = ctypes.c_void_p(None)
        rc = rt.lib.wh_synthesis_timebase_read(fresh, rt.stream(), 1, 8, 81, *([null] * 13))
        assert rc != 0 and b"no time base" in rt.lib.wh_last_error()
    finally:
        _hip.check(rt.lib.wh_ctx_destroy(fresh))
    c = TC.by_name("two_frames_unvoiced")
    b = _Batch(rt, [_utt(c)], c.fs)
    synthesis_timebase_device(rt, b.batch, b.tp_d, b.f0_d, b.vuv_d, c.fs, b.ny, b.t0, b.dt, 8)
    assert synthesis_timebase_read(rt, 1, 8, b.ny)[0]["count"] == 2
    assert synthesis_timebase_read(rt, 1, 8, b.ny)[0]["count"] == 2          # reading changes nothing
    with pytest.raises(_hip.WorldHipError, match="not the time base's"):
        synthesis_timebase_read(rt, 1, 9, b.ny)
    counts, _ = synthesis_plan(rt, b.batch, b.tp_d, b.f0_d, b.vuv_d, c.fs, b.ny, b.t0, b.dt, 8)
    assert counts[0] == 2
    with pytest.raises(_hip.WorldHipError, match="no time base"):
        synthesis_timebase_read(rt, 1, 8, b.ny)
    assert rt.take_flags() == [0] * 16


@pytest.mark.parametrize("fused", [False, True], ids=["inline", "fused"])
@pytest.mark.parametrize("name", TC.names())
def test_case_alone(name, fused):
    c = TC.by_name(name)
    want = ref_of(c, fused)
    limit = TR.low_limit(c.fs, fft_for(c.fs)) if fused else 0.0
    got, flags = run_timebase([_utt(c)], c.fs, want["count"] + 3, limit)
    assert TR.mismatches(got[0], want) == []
    assert np.all(got[0]["weight"][want["same"]] == -1.0)   # one frame: the weight is the marker -1
    assert got[0]["base"] == 0 and flags == [0] * 16


@pytest.mark.parametrize("name", [c.name for c in TC.fused_cases()])
def test_fused_form_on_raw_f0_stage_arrays(name):
    """f0_low_limit > 0: prep_kernel reads the F0 stage's raw output through final_f0 (vuv == 0 -> 0, voiced below
    3 fs / (fft_size - 3) -> 500 Hz; at the limit and above: unchanged)"""
    c = {c.name: c for c in TC.fused_cases()}[name]
    want = ref_of(c, True)
    got, flags = run_timebase([_utt(c)], c.fs, want["count"] + 3, TR.low_limit(c.fs, c.fft_size))
    assert TR.mismatches(got[0], want) == [] and flags == [0] * 16
    if name == "invariant":  # the rule changes nothing here: the two forms give identical bits
        inline, flags = run_timebase([_utt(c)], c.fs, want["count"] + 3, 0.0)
        assert TR.mismatches(inline[0], want) == [] and flags == [0] * 16
        for k in TR.INT_FIELDS + TR.BIT_FIELDS:
            assert inline[0][k].tobytes() == got[0][k].tobytes(), k


# ---- ragged batches ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fs", sorted({c.fs for c in TC.cases()}))
def test_all_cases_of_a_rate_as_one_ragged_batch(fs):
    """every utterance's fields are what it gets alone (= the reference's), bit for bit, whatever its neighbours; p_base
    is the exclusive prefix of the counts"""
    group = [c for c in TC.cases() if c.fs == fs]
    if fs == 16000:  # a second utterance at the odd rates too, so that no batch is a batch of one
        extra = []
    else:
        extra = [TC.Case(c.name + "_again", c.fs, c.tp[: len(c.tp) // 2], c.f0[: len(c.tp) // 2], c.vuv[: len(c.tp) // 2],
                         "", None) for c in group]
    group = group + extra
    for order in (list(range(len(group))), list(range(len(group)))[::-1]):
        cs = [group[i] for i in order]
        wants = [ref_of(c) for c in cs]
        cap = max(w["count"] for w in wants) + 1
        got, flags = run_timebase([_utt(c) for c in cs], fs, cap)
        assert flags == [0] * 16
        base = 0
        for c, g, w in zip(cs, got, wants):
            assert TR.mismatches(g, w) == [], c.name
            assert g["base"] == base, c.name
            base += w["count"]


# ---- wh_synthesis_plan and wh_synthesis' pulse_count_out ---------------------------------------------------------------

def _spectra(name, nf, fft_size=1024):
    rng = np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)
    k = fft_size // 2 + 1
    spec = 1e-4 * (1.0 + 0.5 * np.sin(np.arange(k)[None, :] / 40.0 + rng.uniform(0, 6, (nf, 1)))) ** 2
    ap = rng.uniform(0.05, 0.6, (nf, 1)) * np.ones((1, k))
    return spec, ap


def run_decode(cs, fs, cap, noise=None, fft_size=1024):
    """wh_synthesis itself into a buffer pre-filled with NaN -> (per-utterance samples, pulse_count_out, flags)"""
    from world import _hip

    rt = _rt()
    rt.take_flags()
    b = _Batch(rt, [_utt(c) for c in cs], fs)
    sa = [_spectra(c.name, len(c.tp), fft_size) for c in cs]
    spec_d = rt.to_device(np.concatenate([s for s, _ in sa]))
    ap_d = rt.to_device(np.concatenate([a for _, a in sa]))
    y_off = np.concatenate([[0], np.cumsum(b.ny)]).astype(np.int64)
    y = rt.torch.full((int(y_off[-1]),), float("nan"), dtype=rt.torch.float64, device=rt.device)
    counts = rt.torch.full((b.n,), -1, dtype=rt.torch.int32, device=rt.device)
    vp = ctypes.c_void_p
    noise_d, noff_p = None, vp(None)
    if noise is not None:
        noff = np.concatenate([[0], np.cumsum([len(z) for z in noise])]).astype(np.int64)
        noise_d = rt.to_device(np.concatenate(noise))
        noff_p = noff.ctypes.data_as(vp)
    t0 = np.ascontiguousarray(b.t0, dtype=np.float64)
    dt = np.ascontiguousarray(b.dt, dtype=np.float64)
    _hip.check(rt.lib.wh_synthesis(rt.ctx, rt.stream(), b.batch.handle, rt.ptr(b.tp_d), rt.ptr(b.f0_d), rt.ptr(b.vuv_d),
                                   rt.ptr(spec_d), rt.ptr(ap_d), float(fs), int(fft_size), y_off.ctypes.data_as(vp),
                                   t0.ctypes.data_as(vp), dt.ctypes.data_as(vp), int(cap), rt.ptr(noise_d), noff_p, 0,
                                   rt.ptr(y), rt.ptr(counts)))
    flags = rt.take_flags()
    yh = y.cpu().numpy()
    return [yh[y_off[u]:y_off[u + 1]] for u in range(b.n)], counts.cpu().numpy(), flags


@pytest.mark.parametrize("name", TC.names())
def test_plan_and_pulse_count_out_agree_with_the_reference(name):
    """the two calls a host sizes its noise with: the pulse count, and sum(max(3, noise_size)) = the reference's randn
    draws; with the capacity the facade uses (safe_pulse_cap)"""
    from world.synthesis import safe_pulse_cap, synthesis_plan

    c = TC.by_name(name)
    want = ref_of(c)
    rt = _rt()
    rt.take_flags()
    b = _Batch(rt, [_utt(c)], c.fs)
    cap = safe_pulse_cap(b.ny)
    assert cap >= want["count"]
    counts, draws = synthesis_plan(rt, b.batch, b.tp_d, b.f0_d, b.vuv_d, c.fs, b.ny, b.t0, b.dt, cap)
    assert int(counts[0]) == want["count"] and int(draws[0]) == want["draws"]
    assert rt.take_flags() == [0] * 16
    _, pc, flags = run_decode([c], c.fs, min(cap, want["count"] + 16), fft_size=fft_for(c.fs))
    assert int(pc[0]) == want["count"]
    assert flags[:4] == [0] * 4  # (the row region of the overlap-add may still overflow at fs / 2: slot 4, not this test's)


# ---- capacity ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["const_71hz", "const_7000hz", "chirp_55_1900", "two_frames_unvoiced"])
def test_capacity_clip_keeps_the_first_records(name):
    """pulse_cap = P - 1 / P / P + 1 with P the reference's count.  At P - 1 the flag is raised, the count is clipped and
    the first P - 1 records are the reference's — but for the last kept pulse's noise_size, which the code DEFINES as 0:
    pulse_frames_kernel (and pulse_finish_kernel's noise offsets) take "the next pulse" among the kept ones, so the last
    kept pulse is its own successor, exactly like the reference's last pulse.  Its noise offset is an exclusive prefix and
    is not affected.  At P: no flag, everything equal."""
    c = TC.by_name(name)
    want = ref_of(c)
    p = want["count"]
    got, flags = run_timebase([_utt(c)], c.fs, p - 1)
    assert _raised(flags) == _flags(PULSE_OVERFLOW=1)
    clipped = dict(want, noise_size=want["noise_size"].copy())
    clipped["noise_size"][p - 2] = 0
    assert got[0]["noise_size"][-1] == 0
    assert TR.mismatches(got[0], clipped, n=p - 1) == []
    for cap in (p, p + 1):
        got, flags = run_timebase([_utt(c)], c.fs, cap)
        assert flags == [0] * 16, cap
        assert TR.mismatches(got[0], want) == [], cap


def test_capacity_clip_in_a_batch_touches_only_the_overflowing_utterance():
    cs = [TC.by_name(n) for n in ("const_71hz", "chirp_55_1900", "const_40hz", "const_500hz")]
    wants = [ref_of(c) for c in cs]
    cap = wants[1]["count"] - 1
    assert all(w["count"] < cap for i, w in enumerate(wants) if i != 1)
    got, flags = run_timebase([_utt(c) for c in cs], 16000, cap)
    assert _raised(flags) == _flags(PULSE_OVERFLOW=1)
    clipped = dict(wants[1], noise_size=wants[1]["noise_size"].copy())
    clipped["noise_size"][cap - 1] = 0
    assert TR.mismatches(got[1], clipped, n=cap) == []
    for i in (0, 2, 3):
        assert TR.mismatches(got[i], wants[i]) == [], cs[i].name
    assert [g["base"] for g in got] == [0, wants[0]["count"], wants[0]["count"] + cap, wants[0]["count"] + cap + wants[2]["count"]]
    # exactly full: utterance 3 has the most pulses of a batch whose capacity is its count
    cs2 = [cs[0], cs[3], cs[2]]
    got, flags = run_timebase([_utt(c) for c in cs2], 16000, wants[3]["count"])
    assert flags == [0] * 16
    for g, w in zip(got, [wants[0], wants[3], wants[2]]):
        assert TR.mismatches(g, w) == []


# ---- no pulse -----------------------------------------------------------------------------------------------------------

def _host_noise(c, want):
    n = want["draws"] if want is not None else 8
    return np.random.RandomState(zlib.crc32(c.name.encode()) & 0xFFFF).randn(n)


def test_no_pulse_alone():
    """two frames 1 ms apart: 17 samples, no phase wrap (the reference asserts).  WH_FLAG_NO_PULSE, count 0, and every
    sample of the decode is WRITTEN (zero): the callers hand wh_synthesis uninitialised memory."""
    c = TC.NO_PULSE
    got, flags = run_timebase([_utt(c)], c.fs, 4)
    assert _raised(flags) == _flags(NO_PULSE=1)
    assert got[0]["count"] == 0 and len(got[0]["pidx"]) == 0 and len(got[0]["phase"]) == 17
    t = np.arange(c.tp[0], c.tp[-1] + 1 / c.fs, 1 / c.fs)
    assert np.array_equal(got[0]["phase"].view(np.int64), np.cumsum(2 * np.pi * np.full(len(t), 500.0) / c.fs).view(np.int64))
    assert not got[0]["vuv_s"].any()
    ys, pc, flags = run_decode([c], c.fs, 4, noise=[_host_noise(c, None)])
    assert _raised(flags) == _flags(NO_PULSE=1) and int(pc[0]) == 0
    assert len(ys[0]) == 17 and np.array_equal(ys[0], np.zeros(17))


def test_no_pulse_between_two_ordinary_utterances():
    a, z = TC.by_name("const_71hz"), TC.by_name("fractional_vuv")
    cs = [a, TC.NO_PULSE, z]
    wa, wz = ref_of(a), ref_of(z)
    cap = max(wa["count"], wz["count"]) + 2
    got, flags = run_timebase([_utt(c) for c in cs], 16000, cap)
    assert _raised(flags) == _flags(NO_PULSE=1)
    assert got[1]["count"] == 0 and got[1]["base"] == wa["count"] == got[2]["base"]
    assert TR.mismatches(got[0], wa) == [] and TR.mismatches(got[2], wz) == []
    noise = [_host_noise(a, wa), _host_noise(TC.NO_PULSE, None), _host_noise(z, wz)]
    ys, pc, flags = run_decode(cs, 16000, cap, noise=noise)
    assert _raised(flags) == _flags(NO_PULSE=1) and pc.tolist() == [wa["count"], 0, wz["count"]]
    assert np.array_equal(ys[1], np.zeros(17))
    for i, c in ((0, a), (2, z)):
        solo, pcs, fl = run_decode([c], 16000, cap, noise=[noise[i]])
        assert fl == [0] * 16 and int(pcs[0]) == pc[i]
        assert np.all(np.isfinite(solo[0])) and np.max(np.abs(solo[0])) > 0
        assert np.array_equal(ys[i], solo[0]), c.name


# ---- Requiem shares the pulses ---------------------------------------------------------------------------------------------

def _requiem_dict(c, nb=3):
    spec, _ = _spectra(c.name, len(c.tp))
    rng = np.random.RandomState(zlib.crc32(c.name.encode()) & 0xFFF)
    return {"f0": c.f0, "vuv": c.vuv, "temporal_positions": c.tp, "spectrogram": np.ascontiguousarray(spec.T),
            "aperiodicity": rng.uniform(-25.0, -3.0, (nb, len(c.tp))), "fs": c.fs, "is_requiem": True}


def _requiem_decode(wb, dicts, seeds, cap, cursor=None):
    from world.batch import BatchEncoding

    wb.rt.take_flags()
    enc = BatchEncoding.from_dicts(wb.rt, dicts)
    y, off = wb.decode_device(enc, seeds=seeds, pulse_cap=cap, cursor=cursor, check=False)
    flags = wb.rt.take_flags()
    y = y.cpu().numpy()
    return [y[off[u]:off[u + 1]] for u in range(len(dicts))], flags


@pytest.mark.parametrize("middle", ["exact_capacity", "no_pulse"])
def test_requiem_entry_shares_the_pulses(middle):
    """wh_synthesis_requiem places its pulses with the same launch_pulses (its audio pins their indices elsewhere): here
    only the flags at the exactly full capacity and for a pulse-less utterance, and that a neighbour's samples are its
    solo decode's."""
    from world.batch import WorldBatch
    from world.get_seeds_signals import get_seeds_signals_device
    from world.synthesisRequiem import _advance

    fs = 16000
    a, z = TC.by_name("const_71hz"), TC.by_name("fractional_vuv")
    mid = TC.by_name("const_500hz") if middle == "exact_capacity" else TC.NO_PULSE
    cs = [a, mid, z]
    counts = [ref_of(c)["count"] if c is not TC.NO_PULSE else 0 for c in cs]
    cap = max(counts)
    assert middle == "no_pulse" or counts[1] == cap > max(counts[0], counts[2])
    wb = WorldBatch()
    seeds = get_seeds_signals_device(fs, seed=5)
    nlen, nb = seeds["noise_d"].shape
    dicts = [_requiem_dict(c, nb) for c in cs]
    ys, flags = _requiem_decode(wb, dicts, seeds, cap)
    assert _raised(flags) == (_flags(NO_PULSE=1) if middle == "no_pulse" else [0] * 16)
    cur = np.zeros(nb)
    for u, c in enumerate(cs):
        if c is not TC.NO_PULSE:
            solo, fl = _requiem_decode(wb, [dicts[u]], seeds, cap, cursor=cur.copy())
            assert fl == [0] * 16
            assert np.all(np.isfinite(solo[0])) and np.max(np.abs(solo[0])) > 0
            assert np.array_equal(ys[u], solo[0]), c.name
        cur = _advance(cur, len(ys[u]), nlen)
