"""GPU: the phase accumulator's scan (wh_cumsum_exact) equals np.cumsum BIT FOR BIT — it is a parallel integer
prefix sum per binade of the running sum, so the cases that matter are binade crossings, exact rounding ties,
leading zeros and segment lengths around the tile size."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def run_segments(segs):
    from world import _hip

    rt = _hip.Runtime.get()
    off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    d = rt.to_device(np.concatenate(segs) if len(segs) else np.zeros(0))
    _hip.check(rt.lib.wh_cumsum_exact(rt.ctx, rt.stream(), rt.ptr(d), off.ctypes.data_as(ctypes.c_void_p), len(segs)))
    out = d.cpu().numpy()
    return [out[off[i]:off[i + 1]] for i in range(len(segs))]


def test_matches_numpy_cumsum_bitwise():
    rng = np.random.RandomState(1234)
    segs = []
    # phase-increment-like data: 2*pi*f/fs with slowly varying f, long enough for ~17 binades and a dozen ties
    t = np.arange(400001)
    segs.append(2 * np.pi * (120 + 40 * np.sin(t / 9000.0)) / 16000.0)
    segs.append(np.full(160001, 2 * np.pi * 500 / 16000.0))          # the unvoiced default: a constant increment
    segs.append(rng.uniform(0.0, 1.0, 70000))                         # arbitrary magnitudes
    segs.append(10.0 ** rng.uniform(-12, 3, 50000))                   # 15 decades: crossings everywhere
    segs.append(np.concatenate([np.zeros(37), rng.uniform(0, 1e-3, 5000)]))  # leading zeros
    for n in (0, 1, 2, 31, 32, 33, 2047, 2048, 2049, 4096, 4097):     # around the tile / lane-run sizes
        segs.append(rng.uniform(0.01, 0.1, n))
    # exact ties: increments that are odd multiples of half an ulp of the running sum
    x = np.full(30000, 0.75)
    x[1::2] = 2.0 ** -45 * 3          # sum ~ 1e4 -> ulp 2^-39: these land on .5-ulp boundaries again and again
    segs.append(x)
    y = np.ones(5000)
    y[::3] = 2.0 ** -42               # ulp of sums in [2^10, 2^11) is 2^-42: half-ulp ties need 2^-43 ...
    y[1::3] = 2.0 ** -43
    segs.append(y)
    got = run_segments(segs)
    for g, s in zip(got, segs):
        want = np.cumsum(s)
        assert g.shape == want.shape
        assert np.array_equal(g.view(np.int64), want.view(np.int64))


def test_many_segments_ragged():
    rng = np.random.RandomState(7)
    segs = [rng.uniform(0.02, 0.3, rng.randint(1, 9000)) for _ in range(40)]
    for g, s in zip(run_segments(segs), segs):
        assert np.array_equal(g.view(np.int64), np.cumsum(s).view(np.int64))


# ---- the sizes the scan switches on: kXTile = 4096 samples per tile, more than 64 tiles -> the tile-parallel passes --------

X_TILE, X_MIN_TILES = 4096, 64


def _assert_bitwise(segs):
    for i, (g, s) in enumerate(zip(run_segments(segs), segs)):
        want = np.cumsum(s)
        assert g.shape == want.shape, i
        assert np.array_equal(g.view(np.int64), want.view(np.int64)), (i, len(s))


def test_lengths_around_the_tile_and_the_path_switch():
    """one and two tiles of 4096 +- 1; 64 tiles - 1, 64 tiles (the last length on the one-workgroup path), 64 tiles + 1 (the
    first on the tile-parallel path: its last tile holds one element) and 65 tiles — long and short in one call"""
    rng = np.random.RandomState(99)
    lens = [4095, 4096, 4097, 8191, 8192, 8193,
            X_MIN_TILES * X_TILE - 1, X_MIN_TILES * X_TILE, X_MIN_TILES * X_TILE + 1, (X_MIN_TILES + 1) * X_TILE]
    _assert_bitwise([rng.uniform(0.01, 0.1, n) for n in lens])
    # the same lengths of phase increments that cross binades inside the last tile
    _assert_bitwise([2 * np.pi * (90 + 60 * np.sin(np.arange(n) / 5000.0)) / 16000.0 for n in lens[::-1]])


def test_long_path_patterns():
    """the tile-parallel passes on what they must flag or verify: exact ties (early in the sequence and in the binade the
    sum ends in), a zero carry across a whole tile (5 000 leading zeros), 15 decades, the unvoiced default's constant"""
    from _timebase_cases import scan_patterns

    pats = scan_patterns(300000, zeros=5000)
    assert all(len(x) > X_MIN_TILES * X_TILE and x.min() >= 0 for _, x in pats)
    _assert_bitwise([x for _, x in pats])


def test_long_and_short_segments_mixed_in_one_call():
    from _timebase_cases import scan_patterns

    rng = np.random.RandomState(5)
    long_ = [x for _, x in scan_patterns(X_MIN_TILES * X_TILE + 777, zeros=4200)]
    short = [x for _, x in scan_patterns(9000, zeros=4200)] + [rng.uniform(0, 1, n) for n in (0, 1, 4096, 70000)]
    segs = []
    for i in range(max(len(long_), len(short))):  # interleaved: the two paths split the call's segments between them
        segs += long_[i:i + 1] + short[i:i + 1]
    _assert_bitwise(segs)
