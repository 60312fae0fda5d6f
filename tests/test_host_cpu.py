"""CPU-only tests of the product's host side: C-ABI export surface, host tables, seeds, sharding, and
the 'fail loudly without a GPU' rule.  No compute call reaches the device."""
import os
import random
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from world import _hip

    header = open(os.path.join(ROOT, "include", "world_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(wh_[a-z0-9_]+)\s*\(", header))
    assert len(declared) >= 20
    lib = _hip.load_library()
    missing = [n for n in sorted(declared) if not hasattr(lib, n)]
    assert not missing, missing
    assert declared == set(_hip.SIGNATURES), (declared ^ set(_hip.SIGNATURES))
    assert lib.wh_version() >= 100
    assert lib.wh_num_frames(160000, 16000.0, 5.0) == 2001
    assert lib.wh_d4c_bands(16000.0, 0) == 1 and lib.wh_d4c_bands(48000.0, 1) == 5


def test_every_launch_goes_through_the_helper():
    """wh::launch / WH_LAUNCH (csrc/wh_host.h) is the one place that brackets a kernel for the profile, launches it and
    reads the runtime's error: no other file launches by hand, times by hand or checks by hand."""
    import glob

    csrc = os.path.join(ROOT, "python-world_amd", "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")))
    assert len(files) > 40 and os.path.join(csrc, "wh_host.h") in files
    raw = ("hipLaunchKernelGGL", "<<<", "KernelTimer", "WH_LAUNCH_CHECK", "hipGetLastError")
    found = []
    for path in files:
        if os.path.basename(path) == "wh_host.h":
            continue
        text = open(path).read()
        found += [(os.path.basename(path), word) for word in raw if word in text]
    assert not found, found


def test_every_workspace_layout_goes_through_the_carver():
    """wh::Carve / wh::Region (csrc/wh_arena.h) is the one place that rounds a scratch region to 256 bytes and turns an
    offset into a typed pointer: no other file rounds by hand or casts `workspace + offset` by hand."""
    import glob

    csrc = os.path.join(ROOT, "python-world_amd", "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")))
    assert len(files) > 40 and os.path.join(csrc, "wh_arena.h") in files
    found = []
    for path in files:
        if os.path.basename(path) == "wh_arena.h":
            continue
        for n, line in enumerate(open(path).read().splitlines(), 1):
            if "& ~(size_t)255" in line or re.search(r"reinterpret_cast<.*\((ws|d_ws) \+", line):
                found.append((os.path.basename(path), n, line.strip()))
    assert not found, found


def test_no_cpu_fallback_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from world import _hip
    from world.cheaptrick import cheaptrick

    with pytest.raises(_hip.WorldHipError):
        cheaptrick(np.zeros(1600), 16000, {"f0": np.zeros(21), "vuv": np.zeros(21),
                                           "temporal_positions": np.arange(21) * 0.005})


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: nothing under python-world_amd/ may import or execute it."""
    pkg = os.path.join(ROOT, "python-world_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), (dirpath, f)
                assert "/root/reference" not in src, (dirpath, f)


def test_host_tables_match_reference_fixture(golden):
    from world import _tables

    g = golden("syn16k")
    tb = _tables.dio_tables(71, 800, 2, 4000)
    assert list(tb["band_bias"]) == list(g["dio_index_bias"]), "Nuttall argmax tie differs on this host (SURVEY Q5)"
    assert list(tb["band_len"]) == [80, 56, 40, 28, 20, 16, 8]
    t = golden("tables")
    for fs, n in ((16000, 160000), (22050, 102400), (48000, 480000)):
        nf = _tables.frame_count(n, fs, 5)
        assert nf == int(t["F_%d" % fs])
        from world.synthesis import time_axis_params
        tp = _tables.frame_times(nf, 5)
        assert time_axis_params(tp, fs)[0] == int(t["Ny_%d" % fs])
        assert time_axis_params(tp * 2.0, fs)[0] == int(t["Ny2_%d" % fs])
    qt = _tables.quantised_times(16000, 340)
    assert qt[340 + 4] == float("%.4f" % (4 / 16000)) and len(qt) == 681
    hv = _tables.harvest_tables(16000, 71, 800)
    assert len(hv["band_f0"]) == 152 and hv["r"] == 2 and int(hv["band_half"].max()) == 246


@pytest.mark.parametrize("tag", ["syn16k", "syn48k"])
def test_seeds_match_reference(golden, tag):
    from world.get_seeds_signals import get_seeds_signals

    g = golden(tag)
    random.seed(int(g["seed"]))
    np.random.seed(int(g["seed"]))
    s = get_seeds_signals(int(g["fs"]))
    assert s["pulse"].shape == g["seeds_pulse"].shape and s["noise"].shape == g["seeds_noise"].shape
    assert np.max(np.abs(s["pulse"] - g["seeds_pulse"])) < 1e-15
    assert np.max(np.abs(s["noise"] - g["seeds_noise"])) < 1e-13


def test_facade_surface():
    from world import main

    W = main.World()
    for name in ("get_f0", "get_spectrum", "encode_w_gvn_f0", "encode", "scale_pitch", "set_pitch", "scale_duration",
                 "modify_duration", "warp_spectrum", "decode"):
        assert callable(getattr(W, name))
    dat = {"f0": np.array([100.0, 200.0]), "temporal_positions": np.array([0.0, 0.005])}
    assert W.scale_pitch(dat, 1.5) is dat and np.array_equal(dat["f0"], [150.0, 300.0])
    assert W.scale_duration(dat, 2.0) is dat and np.array_equal(dat["temporal_positions"], [0.0, 0.01])
    with pytest.raises(NotImplementedError):
        W.set_pitch(dat, None, None)
    with pytest.raises(Exception):
        W.encode(16000, np.zeros(1600), f0_method="nope")


def test_encode_batch_mirrors_encode_signature():
    """encode_batch must default to the same estimator and parameters as encode()."""
    import inspect

    from world import main

    a = inspect.signature(main.World.encode).parameters
    b = inspect.signature(main.World.encode_batch).parameters
    # batch-only: encode() always returns 'ps spectrogram', the batch keeps it on request; `devices`: one host thread per GPU
    extra = ("want_ps", "devices")
    assert [k for k in a if k not in ("self", "fs", "x")] == [k for k in b if k not in ("self", "fs", "xs") + extra]
    for k in b:
        if k not in ("self", "fs", "xs") + extra:
            assert a[k].default == b[k].default, k
    assert b["want_ps"].default is False and b["devices"].default is None
    assert b["f0_method"].default == "harvest"


def test_sharded_batch_before_encode_is_none():
    from world.distributed import ShardedWorldBatch

    sb = ShardedWorldBatch(backend=object())
    assert sb.enc is None and sb.decode() is None and sb.gather_f0() == []


def test_shard_ranges_properties():
    from world.distributed import shard_ranges

    rng = np.random.RandomState(0)
    for _ in range(200):
        n = rng.randint(1, 40)
        w = rng.randint(1, 9)
        lens = rng.randint(1000, 200000, size=n)
        r = shard_ranges(lens, w)
        assert len(r) == w and r[0][0] == 0 and r[-1][1] == n
        for a, b in zip(r[:-1], r[1:]):
            assert a[1] == b[0] and a[0] <= a[1]
        if n >= w:
            assert all(e > s for s, e in r)
    assert shard_ranges([160000] * 1024, 8) == [(128 * i, 128 * (i + 1)) for i in range(8)]


def test_lane_split_and_bench_bytes():
    """WorldBatchLanes deals utterances by the rank-sharding rule; bench.py's algorithmic bytes per frame are the
    SURVEY 8(d) figures (17 744 B/frame for the whole path at 16 kHz / fft 1024)."""
    import bench
    from world.batch import WorldBatchLanes

    assert WorldBatchLanes.split([160000] * 64, 2) == [(0, 32), (32, 64)]
    parts = WorldBatchLanes.split([1000, 50000, 2000, 30000, 700], 3)
    assert parts[0][0] == 0 and parts[-1][1] == 5 and all(a[1] == b[0] for a, b in zip(parts[:-1], parts[1:]))
    per_kernel, path = bench.algo_bytes_per_frame(16000, 1024)
    assert path == 17744 and per_kernel["d4c_kernel"] == 640 + 24 + 4104
    per48, path48 = bench.algo_bytes_per_frame(48000, 2048, 2.0)
    assert per48["d4c_kernel"] == 1920 + 24 + 8200 and path48 == 1920 + 3840 + 48 + 4 * 8200


def test_arange_length_memo_is_numpy():
    """time_axis_params memoises len(np.arange(...)) — the float-arange quirk (Q9) must survive the cache."""
    from world.synthesis import _arange_len

    for start, stop, step in ((0.0, 10.0 + 1 / 48000, 1 / 48000), (0.0, 2.0 + 1 / 16000, 1 / 16000),
                              (0.005, 1.2 + 1 / 22050, 1 / 22050)):
        for _ in range(2):
            assert _arange_len(start, stop, step) == len(np.arange(start, stop, step))


def test_refinement_windows_do_not_depend_on_the_frame_time():
    """The tabulated windows of hv_refine_kernel / stonemask_tab_kernel rest on one observation: the reference's
    index_raw enters the window argument un-truncated, so the frame time cancels.  Checked here against the oracle's
    own expressions (oracle/pitch_harvest.py:134-136 = world/harvest.py:178-183; oracle/pitch_dio.py stonemask =
    world/stonemask.py:38-45) for frame times on and off the sample grid, at the decimated rates 8000 and 7350 Hz and
    the full rates 16 / 44.1 / 48 kHz."""
    import math

    from oracle import common as C
    from oracle import pitch_dio

    rng = np.random.RandomState(5)
    # Harvest: common = pi*((index_raw - 1)/fs - t0)/(L/fs), index_raw = half_up((t0 + k/fs)*fs + 0.001)
    for fs_d in (8000.0, 7350.0):
        for _ in range(40):
            h = int(rng.randint(8, 190))
            t0 = float(rng.uniform(0.05, 59.0)) if rng.rand() < 0.5 else float(rng.randint(50, 59000)) / 1000
            k = np.arange(-h, h + 1)
            ln = 2 * h + 1
            idx_raw = C.half_up((t0 + k / fs_d) * fs_d + 0.001)
            common = math.pi * ((idx_raw - 1) / fs_d - t0) / (ln / fs_d)
            ref = 0.42 + 0.5 * np.cos(2 * common) + 0.08 * np.cos(4 * common)
            j = np.arange(ln)
            c = np.cos(math.pi * (2 * ((j - h + (0.001 + 0.5) - 1.0) / fs_d) / (ln / fs_d)))   # wh_hv_refine.hip, host table
            tab = 0.42 + 0.5 * c + 0.08 * (2 * c * c - 1)
            assert np.max(np.abs(tab - ref)) < 5e-12 * max(1.0, t0)   # the cancellation noise of the reference itself (measured: 3e-13 * t0)
    # StoneMask: wt = (index_raw - 1)/fs - t0 with index_raw = half_up((t0 + bt)*fs), bt the 4-decimal quantised times
    for fs in (16000.0, 44100.0, 48000.0):
        for _ in range(30):
            h = int(rng.randint(20, 600))
            t0 = float(rng.uniform(0.1, 30.0)) if rng.rand() < 0.5 else float(rng.randint(20, 6000)) * 0.005
            qt = pitch_dio.quantised_time_table(fs, h)
            bt = qt[np.arange(-h, h + 1) + h]
            idx_raw = C.half_up((t0 + bt) * fs)
            wlit = (2 * h + 1) / fs
            ref = np.cos(2 * math.pi * ((idx_raw - 1) / fs - t0) / wlit)
            tab = np.cos(math.pi * ((bt - 0.5 / fs) * (2.0 / wlit)))                           # wh_stonemask.hip, host table
            assert np.max(np.abs(tab - ref)) < 2e-11 * max(1.0, t0)  # measured: 1e-12 * t0


def test_prefetched_time_base_validity_rules():
    """BatchEncoding.timebase_for (host logic of the decode-time-base prefetch): valid only for the tensors it was
    computed from, untouched (in-place version counters), for the shared time-base context's latest prefetch, and for
    the same pulse capacity."""
    import types

    import torch

    from world.batch import BatchEncoding

    tb_rt = types.SimpleNamespace(timebase_generation=3)
    owner = types.SimpleNamespace(_tb_rt=tb_rt)
    other_owner = types.SimpleNamespace(_tb_rt=types.SimpleNamespace(timebase_generation=3))
    nf = 5
    enc = BatchEncoding(None, None, 16000, torch.arange(nf, dtype=torch.float64) * 0.005, torch.full((nf,), 100.0, dtype=torch.float64),
                        torch.ones(nf, dtype=torch.float64), None, None, 1024, False, 5)
    assert enc.timebase_for(owner, None) is None  # nothing prefetched
    enc._timebase = {"generation": 3, "rt": tb_rt, "pulse_cap": 77, "stamp": enc._stamp()}
    assert enc.timebase_for(owner, None) is enc._timebase
    assert enc.timebase_for(owner, 77) is enc._timebase and enc.timebase_for(owner, 78) is None
    assert enc.timebase_for(other_owner, None) is None       # another (device, lane)'s time-base context
    tb_rt.timebase_generation = 4                              # a later prefetch took the context over
    assert enc.timebase_for(owner, None) is None
    tb_rt.timebase_generation = 3
    fresh = lambda: {"generation": 3, "rt": tb_rt, "pulse_cap": 77, "stamp": enc._stamp()}  # noqa: E731
    enc.scale_pitch(1.5)                                       # the modifiers drop the time base themselves ...
    assert enc._timebase is None and enc.timebase_for(owner, None) is None
    enc._timebase = fresh()
    enc.scale_duration(2.0)
    assert enc._timebase is None
    enc._timebase = fresh()
    enc.temporal_positions = enc.temporal_positions.clone()
    assert enc._timebase is None
    enc._timebase = fresh()
    enc.f0 *= 1.01                                             # ... an in-place edit behind the object's back bumps the
    assert enc.timebase_for(owner, None) is None               # tensor's version counter
    enc._timebase = fresh()
    assert enc.timebase_for(owner, None) is not None
    enc.f0 = enc.f0.clone()                                    # a new tensor: another pointer
    assert enc.timebase_for(owner, None) is None
    with torch.inference_mode():                               # no version counters: no time base is trusted
        enc.f0 = torch.ones(nf, dtype=torch.float64)
    assert enc._stamp() is None
    enc._timebase = {"generation": 3, "rt": tb_rt, "pulse_cap": 77, "stamp": None}
    assert enc.timebase_for(owner, None) is None


def test_table_tag_is_content_identity():
    from world._hip import table_tag

    a = np.arange(12.0).reshape(3, 4)
    assert table_tag(a) == table_tag(a.copy()) and table_tag(a) != 0 and table_tag(a) % 2 == 1
    assert table_tag(a) != table_tag(a.reshape(4, 3))          # same bytes, another shape
    b = a.copy()
    b[1, 2] += 1e-9
    assert table_tag(a) != table_tag(b)
    assert table_tag(a, b) != table_tag(b, a) and table_tag(a) < 2 ** 63


def test_encoding_dict_materialises_on_read_and_remembers_it():
    """world.batch.EncodingDict (the dicts World.encode_batch returns) on a stub encoding, no GPU: a real dict with
    encode()'s keys; a dense value is downloaded by the first read — whatever the way of reading — and only a value
    that was never handed out is still 'resident' for decode_batch (resident_rows)."""
    import contextlib
    import copy
    import pickle
    import types

    import torch

    from world.batch import EncodingDict, BatchEncoding

    downloads = []

    torch_mod = torch

    class StubRt:
        index = 0
        torch = torch_mod

        def on_stream(self):
            return contextlib.nullcontext()

        def to_host(self, t, transpose=False):
            downloads.append(tuple(t.shape))
            return (t.transpose(0, 1) if transpose else t).contiguous().numpy().copy()

    nf, k = [4, 3], 5
    fo = np.array([0, 4, 7])
    spec = torch.arange(7 * k, dtype=torch.float64).reshape(7, k)
    ap = spec + 0.5
    rt = StubRt()
    enc = BatchEncoding(rt, types.SimpleNamespace(frame_off=fo, n_utt=2), 16000, torch.arange(7, dtype=torch.float64) * 0.005,
                        torch.full((7,), 100.0, dtype=torch.float64), torch.ones(7, dtype=torch.float64), spec, ap, 8, False, 5)
    dats = enc.to_dicts(lazy=True)
    assert all(type(d) is EncodingDict and isinstance(d, dict) for d in dats)
    d = dats[1]
    assert list(d.keys()) == ['temporal_positions', 'vuv', 'fs', 'f0', 'aperiodicity', 'spectrogram', 'is_requiem']
    assert 'spectrogram' in d and len(d) == 7 and downloads == []  # membership, length, keys: nothing moves
    assert "resident in HBM" in repr(d) and downloads == []
    assert d['f0'].shape == (3,) and d['fs'] == 16000 and d['is_requiem'] is False and downloads == []
    d['f0'] *= 1.5                                                      # scale_pitch: in place on the host scalars
    assert np.all(d['f0'] == 150.0) and downloads == []
    assert torch.equal(d.resident_rows('spectrogram', rt), spec[4:7])   # decode_batch would take the device rows
    assert d.resident_rows('spectrogram', types.SimpleNamespace(index=1)) is None  # ... not on another device
    s = d['spectrogram']                                                # first read: this utterance's slice, transposed
    assert downloads == [(3, k)] and s.shape == (k, 3) and np.array_equal(s, spec[4:7].numpy().T)
    assert d['spectrogram'] is s and downloads == [(3, k)]              # an ordinary entry from now on
    assert d.resident_rows('spectrogram', rt) is None                   # handed out: may have been edited
    assert d.resident_rows('aperiodicity', rt) is not None              # the other dense value is untouched
    s[...] = 7.0                                                        # in-place edit of the array the caller holds
    assert np.all(d['spectrogram'] == 7.0)
    d['aperiodicity'] = np.zeros((k, 3))                                # replaced without ever being read
    assert d.resident_rows('aperiodicity', rt) is None and downloads == [(3, k)]
    # the other ways of reading: get / items / values / dict() / ** / copy / pop / pickle — each materialises
    for read in (lambda e: e.get('spectrogram'), lambda e: dict(e.items())['spectrogram'], lambda e: e.values()[5],
                 lambda e: dict(e)['spectrogram'], lambda e: {**e}['spectrogram'], lambda e: e.copy()['spectrogram'],
                 lambda e: copy.copy(e)['spectrogram'], lambda e: np.asarray(e['spectrogram']),
                 lambda e: pickle.loads(pickle.dumps(e))['spectrogram'], lambda e: e.pop('spectrogram'),
                 lambda e: e.setdefault('spectrogram', None)):
        e = enc.to_dicts(lazy=True)[0]
        v = read(e)
        assert isinstance(v, np.ndarray) and np.array_equal(v, spec[0:4].numpy().T)
        assert e.resident_rows('spectrogram', rt) is None
    e = enc.to_dicts(lazy=True)[0]
    assert e.get('nothing', 3) == 3 and e.pop('nothing', 4) == 4
    e.update(spectrogram=np.ones((k, 4)))
    assert e.resident_rows('spectrogram', rt) is None and type(pickle.loads(pickle.dumps(e))) is dict
    # the eager form is unchanged: plain dicts, everything downloaded
    plain = enc.to_dicts()
    assert type(plain[0]) is dict and np.array_equal(plain[1]['aperiodicity'], ap[4:7].numpy().T)
    # from_dicts: all-resident in order -> the encoding's own tensors; a read / permuted list -> copies of the rows
    class UpRt(StubRt):
        def make_batch(self, x_off, frame_off):
            return types.SimpleNamespace(frame_off=np.asarray(frame_off), n_utt=len(frame_off) - 1)

        def to_device(self, a, dtype=np.float64):
            return self.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype))

        def to_device_concat(self, arrays):
            return self.torch.from_numpy(np.concatenate([np.asarray(a, dtype=np.float64) for a in arrays]))

    up = UpRt()
    enc.rt = up
    fresh = enc.to_dicts(lazy=True)
    again = BatchEncoding.from_dicts(up, fresh)
    assert again.spectrogram is spec and again.aperiodicity is ap and again.fft_size == 8
    # the per-frame scalars of every utterance, one staged upload: frame times, f0, vuv
    assert torch.equal(again.temporal_positions, torch.arange(7, dtype=torch.float64) * 0.005)
    assert torch.equal(again.f0, torch.full((7,), 100.0, dtype=torch.float64)) and torch.equal(again.vuv, torch.ones(7, dtype=torch.float64))
    swapped = BatchEncoding.from_dicts(up, fresh[::-1])
    assert torch.equal(swapped.spectrogram, torch.cat([spec[4:7], spec[0:4]]))
    fresh[0]['spectrogram'][...] = -1.0                                  # read + edited: uploaded from the host
    mixed = BatchEncoding.from_dicts(up, fresh)
    assert torch.equal(mixed.spectrogram[:4], torch.full((4, k), -1.0, dtype=torch.float64))
    assert torch.equal(mixed.spectrogram[4:], spec[4:7]) and mixed.aperiodicity is ap


def test_philox_seed_for_offset_rekeys_the_utterance_streams():
    """World.decode_batch renders a large batch in consecutive parts; utterance u of a part that starts at utterance
    `base` must draw the noise of utterance base + u of the whole batch.  The device keys a stream with
    seed * A + u * B + 1 mod 2**64 (philox_key, csrc/wh_philox.h): the shifted seed solves that for every u."""
    from world.synthesis import _PHILOX_SEED_MUL as A, _PHILOX_UTT_MUL as B, philox_seed_for_offset

    src = open(os.path.join(os.path.dirname(__file__), "..", "python-world_amd", "csrc", "wh_philox.h")).read()
    assert "return seed * 0x%Xull + u * 0x%Xull + 1;" % (A, B) in src  # the constants are the kernel's
    m = 1 << 64
    key = lambda seed, u: (seed * A + u * B + 1) % m  # noqa: E731
    for seed in (0, 1, 9, 2**63 + 12345, m - 1):
        assert philox_seed_for_offset(seed, 0) == seed
        for base in (1, 32, 511, 70000):
            shifted = philox_seed_for_offset(seed, base)
            assert 0 <= shifted < m
            for u in (0, 1, 31, 1023):
                assert key(shifted, u) == key(seed, base + u)


def test_decode_batch_parts_of_plain_dicts():
    """_decode_groups: one part for small batches, Requiem and callers that steer the checks; two consecutive,
    non-empty parts balanced by frames otherwise."""
    from world import main

    def dat(frames, requiem=False):
        tp = np.arange(frames) * 0.005
        return {'f0': np.zeros(frames), 'temporal_positions': tp, 'fs': 16000, 'is_requiem': requiem}

    big = [dat(2001) for _ in range(64)]               # 64 x 10 s @16 kHz: 82 MB of audio
    assert main.FACADE_SPLIT_BYTES == 16 << 20
    assert main._decode_groups(big, {}) == [(0, 32), (32, 64)]
    assert main._decode_groups(big, {'seed': 3, 'noise': None}) == [(0, 32), (32, 64)]
    assert main._decode_groups(big, {'check': False}) == [(0, 64)]
    assert main._decode_groups(big, {'cursor': np.zeros(3)}) == [(0, 64)]
    assert main._decode_groups([dat(2001, True) for _ in range(64)], {}) == [(0, 64)]
    assert main._decode_groups(big[:1], {}) == [(0, 1)]
    assert main._decode_groups([dat(201) for _ in range(8)], {}) == [(0, 8)]   # 8 s of audio: a single batch
    ragged = [dat(12001)] + [dat(801) for _ in range(30)]
    (a0, a1), (b0, b1) = main._decode_groups(ragged, {})
    assert a0 == 0 and a1 == b0 and b1 == 31 and a1 >= 1


def test_bench_defaults_match_the_contract(monkeypatch):
    """`python bench.py` with no flags: N = 1, config 2 at its BASELINE size, a K / W that finish within minutes, two
    whole steps in flight (and `--in-flight 1` available); config 5 switches to its own size."""
    import sys

    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py"])
    a = bench.parse()
    assert (a.gpus, a.config, a.utts, a.seconds, a.scaling, a.in_flight, a.lanes) == (1, 2, 64, 10.0, "weak", 2, 1)
    assert 5 <= a.steps <= 50 and 1 <= a.warmup <= 10 and a.north_star_utts == 1024
    monkeypatch.setattr(sys, "argv", ["bench.py", "--config", "5", "--in-flight", "1"])
    b = bench.parse()
    assert (b.utts, b.seconds, b.in_flight) == (16, 60.0, 1)
    # a plain run times the headline only; --full is everything else, its opt-outs unchanged
    assert not a.full and a.no_cpu_baseline and a.no_extras and a.no_pmc and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-pmc", "--steps", "7", "--dump-outputs", "d"])
    c = bench.parse()
    assert c.full and c.no_pmc and not c.no_cpu_baseline and not c.no_extras and (c.steps, c.dump_outputs) == (7, "d")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def test_bench_dump_outputs_joins_lanes_and_samples_large_arrays(tmp_path, monkeypatch):
    """bench.py --dump-outputs: the lanes' parts of a step's result in utterance order, out_offsets into the joined audio,
    arrays above the per-array budget as seeded stratified row samples (the same rows every run, with their indices),
    everything float32 / float64."""
    import types

    import numpy as np
    import torch

    import bench

    monkeypatch.setattr(bench, "DUMP_ARRAY_BYTES", 4096)

    def lane(nf, ny, u):
        g = torch.Generator().manual_seed(u)
        e = types.SimpleNamespace(temporal_positions=torch.arange(nf, dtype=torch.float64) * 0.005,
                                  f0=torch.rand(nf, generator=g, dtype=torch.float64),
                                  vuv=(torch.rand(nf, generator=g) > 0.5).to(torch.int32),
                                  spectrogram=torch.rand(nf, 33, generator=g, dtype=torch.float64),
                                  aperiodicity=torch.rand(nf, 5, generator=g, dtype=torch.float32))
        return e, (torch.rand(ny, generator=g, dtype=torch.float64), np.array([0, ny // 3, ny], dtype=np.int64))

    (e0, d0), (e1, d1) = lane(300, 2000, 1), lane(200, 1500, 2)
    named = dict(bench.step_outputs(2, ([e0, None, e1], [d0, None, d1])))
    assert named["out_offsets"].tolist() == [0, 666, 2000, 2500, 3500]
    assert torch.equal(named["vuv"], torch.cat([e0.vuv, e1.vuv]))
    runs = []
    for r in range(2):
        bench.dump_outputs(list(named.items()), str(tmp_path / str(r)))
        runs.append({p.name: np.load(p) for p in (tmp_path / str(r)).iterdir()})
    assert runs[0].keys() == runs[1].keys() and all(np.array_equal(runs[0][k], runs[1][k]) for k in runs[0])
    got = runs[0]
    assert {k: v.dtype for k, v in got.items() if not k.endswith("_index.npy")} == {
        "temporal_positions.npy": np.float64, "f0.npy": np.float64, "vuv.npy": np.float64, "spectrogram.npy": np.float64,
        "aperiodicity.npy": np.float32, "out.npy": np.float64, "out_offsets.npy": np.float64}
    assert np.array_equal(got["f0.npy"], named["f0"].numpy()) and "f0_index.npy" not in got       # 4000 B: whole
    for k in ("spectrogram", "out"):
        idx = got[k + "_index.npy"].astype(np.int64)
        assert got[k + ".npy"].nbytes <= 4096 and len(idx) >= 2 and np.all(np.diff(idx) > 0)
        assert np.array_equal(got[k + ".npy"], named[k].numpy()[idx])
    assert [k for k, _ in bench.step_outputs(3, [(e0.f0, e0.vuv), (e1.f0, e1.vuv)])] == ["f0", "vuv"]



def test_requiem_cursor_chain_over_ranges_equals_the_utterance_chain():
    """world.pool hands every device a contiguous range of a Requiem batch; the noise-seed cursor a range starts at is
    computed on the host from the output lengths (world/synthesisRequiem.py:131-141 keeps index[-1]): cutting
    the chain anywhere must give the cursor the single batch reaches there."""
    import numpy as np
    from world.synthesisRequiem import _advance, cursor_after, seed_table_shape
    from world.synthesis import time_axis_params

    fs = 16000
    nlen, nb = seed_table_shape(fs)
    assert (nlen, nb) == (8192, 3)
    rng = np.random.RandomState(4)
    tps = [np.arange(int(n)) * 0.005 for n in rng.randint(40, 900, size=9)]
    cur = np.zeros(nb)
    want = []
    for tp in tps:
        want.append(cur.copy())
        cur = _advance(cur, time_axis_params(tp, fs)[0], nlen)
    for cut in (0, 1, 4, 9):
        c0 = cursor_after(tps[:cut], fs, np.zeros(nb), nlen)
        assert np.array_equal(c0, want[cut] if cut < 9 else cur)
        assert np.array_equal(cursor_after(tps[cut:], fs, c0, nlen), cur)
    tabs = {"noise": np.zeros((4096, 5)), "pulse": np.zeros((1024, 5))}
    assert seed_table_shape(fs, tabs) == (4096, 5)


def test_pool_fails_loudly_without_a_gpu():
    """No CPU fallback behind the thread-per-device driver either: without a GPU the first job raises WorldHipError on the
    caller's thread (and the worker stays usable for the next call)."""
    import numpy as np
    import pytest
    import torch
    from world import _hip
    from world.pool import WorldBatchPool

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(_hip.WorldHipError):
        WorldBatchPool()  # (device discovery)
    pool = WorldBatchPool([0])
    try:
        for _ in range(2):
            with pytest.raises(_hip.WorldHipError):
                pool.encode([np.zeros(16000)], 16000, f0_method="dio")
        assert pool.ranges([10, 10, 10]) == [(0, 3)]
    finally:
        pool.close()


def test_harvest_event_capacity_hints():
    """world.harvest.hinted_event_caps: nothing to add -> None (the library sizes its crossing lists itself: the benchmark
    path); with flat stretches in the host waveforms -> the library's estimate plus one entry per two flat DECIMATED samples
    per list, utterance by utterance; and the setter of the C-ABI refuses nonsense without touching a device."""
    import ctypes
    from types import SimpleNamespace

    from world import _hip, _tables
    from world.harvest import flat_samples, hinted_event_caps

    fs = 16000
    tb = _tables.harvest_tables(fs, 71, 800)
    nb = len(tb["band_f0"])
    assert nb == 152 and int(tb["r"]) == 2
    x = np.random.RandomState(0).randn(16000)
    padded = np.concatenate([np.zeros(4800), x, np.full(1600, 0.25)])
    assert flat_samples(x) == 0 and flat_samples(padded) == 4799 + 1599
    mk = lambda lens, flat: SimpleNamespace(n_utt=len(lens), x_off=np.concatenate([[0], np.cumsum(lens)]), flat_samples=flat)  # noqa: E731
    assert hinted_event_caps(SimpleNamespace(n_utt=1, x_off=np.array([0, 16000])), fs, tb) is None  # (no host arrays seen)
    assert hinted_event_caps(mk([16000], [0]), fs, tb) is None
    assert hinted_event_caps(mk([16000], [100]), fs, tb) is None  # (100 / 4 = 25 entries: inside the estimate's slack)
    caps = hinted_event_caps(mk([16000, len(padded)], [0, flat_samples(padded)]), fs, tb).reshape(2, nb)
    est = lambda n: np.ceil((n // 2 + 2) / 8000.0 * tb["band_f0"] * 3.0).astype(np.int64) + 64  # noqa: E731
    assert np.array_equal(caps[0], est(16000) + 16)
    assert np.array_equal(caps[1], est(len(padded)) + 6398 // 4 + 16)
    assert caps[1].min() > 6398 // 4  # every list can take the flat stretches' sign changes
    lib = _hip.load_library()
    assert lib.wh_harvest_set_event_caps(None, None, 0) != 0            # null context
    assert lib.wh_harvest_event_counts(None, None, None, 0) != 0
    assert b"null" in lib.wh_last_error()


def test_decode_refuses_dicts_whose_arrays_disagree():
    """World.decode / decode_batch index the per-frame arrays by the frame count: arrays of other lengths, dense tensors of
    another layout and batches of mixed rate / path / bin count are refused before anything reaches the device."""
    from world.main import _check_decodable

    F, K = 50, 513
    good = {"temporal_positions": np.arange(F) * 0.005, "f0": np.full(F, 120.0), "vuv": np.ones(F), "fs": 16000,
            "is_requiem": False, "spectrogram": np.ones((K, F)), "aperiodicity": np.ones((K, F))}
    _check_decodable([good, dict(good)])
    for bad in (dict(good, f0=good["f0"][:-3]), dict(good, vuv=np.ones((F, 1))), dict(good, spectrogram=np.ones((F, K))),
                dict(good, aperiodicity=np.ones((K, F - 1))), dict(good, temporal_positions=good["temporal_positions"][:1], f0=good["f0"][:1], vuv=good["vuv"][:1])):
        with pytest.raises(ValueError):
            _check_decodable([bad])
    for other in (dict(good, fs=22050), dict(good, is_requiem=True), dict(good, spectrogram=np.ones((257, F)))):
        with pytest.raises(ValueError):
            _check_decodable([good, other])
    with pytest.raises(KeyError):
        _check_decodable([{k: v for k, v in good.items() if k != "f0"}])


def test_stage_functions_refuse_arrays_of_different_lengths():
    """_hip.same_frames, the guard in front of every per-stage drop-in (cheaptrick, d4c, d4cRequiem, stonemask, synthesis,
    synthesisRequiem): nothing reaches a kernel that would index a short array by the batch's frame count."""
    from world import _hip
    from world.cheaptrick import cheaptrick
    from world.stonemask import stonemask

    assert _hip.same_frames("t", temporal_positions=np.zeros(7), f0=np.zeros(7), vuv=[0] * 7) == 7
    assert _hip.same_frames("t", dense=(("spectrogram", np.zeros((5, 7))),), f0=np.zeros(7)) == 7
    with pytest.raises(ValueError):
        _hip.same_frames("t", temporal_positions=np.zeros(7), f0=np.zeros(6))
    with pytest.raises(ValueError):
        _hip.same_frames("t", f0=np.zeros((7, 1)))
    with pytest.raises(ValueError):
        _hip.same_frames("t", dense=(("spectrogram", np.zeros((7, 5))),), f0=np.zeros(7))
    x = np.zeros(1600)
    with pytest.raises(ValueError):  # (before any device call: holds without a GPU)
        cheaptrick(x, 16000, {"f0": np.full(20, 100.0), "vuv": np.ones(21), "temporal_positions": np.arange(21) * 0.005})
    with pytest.raises(ValueError):
        stonemask(x, 16000, np.arange(21) * 0.005, np.full(20, 100.0))
