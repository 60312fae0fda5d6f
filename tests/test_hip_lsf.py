"""GPU: wh_lpc_levinson, wh_lsf_from_lpc and wh_lsf_envelope (csrc/wh_lsf.hip), each through the C ABI on the input the
reference has for it, compared with tests/_lsf_reference.py bit for bit — there is no tolerance on the three kernels —
and the chain of world.lsf on the committed spectrogram fixtures."""
import os

import numpy as np
import pytest

import _feature_reference as fr
import _lsf_cases as lc
import _lsf_reference as ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# the log-spectral distortion of the rebuilt envelope against the fixture, dB (the issue's table; re-derived below)
TABLE = (("golden_syn16k", 24, 2.158), ("golden_syn16k", 40, 1.559), ("golden_syn16k", 64, 0.984),
         ("golden_syn48k", 40, 3.301), ("golden_syn48k", 64, 2.771))


def _rt():
    from world import _hip

    return _hip.Runtime.get()


def _lsf_flag(flags):
    """1 / 0 for WH_FLAG_LSF; every other flag must be clear."""
    from world import _hip

    assert sum(1 for i, v in enumerate(flags) if v and i != _hip.FLAG_LSF) == 0, flags
    return int(flags[_hip.FLAG_LSF] != 0)


@pytest.fixture(autouse=True)
def flags_are_clear():
    yield
    assert _rt().take_flags() == [0] * 16


# ---- a. shapes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lc.kernel_cases(), ids=lambda c: c.name)
def test_each_kernel_equals_the_reference_bit_for_bit(case):
    """p in {2, 4, 24, 40, 64} x F in {1, 63, 64, 65, 129, 257}: a, E, the reflection coefficients; the cosines and the
    level; the envelope at K in {129, 513, 1025, 2049}.  Every other case keeps inputs and outputs inside wider tensors
    of NaN, which must be neither read nor written."""
    rt = _rt()
    assert lc.compare(lc.run(rt, case), lc.reference(case)) == []
    assert rt.take_flags() == [0] * 16


def test_the_case_list_covers_what_it_says():
    cases = lc.kernel_cases()
    assert {(c.p, c.frames) for c in cases} == {(p, f) for p in lc.ORDERS for f in lc.FRAMES}
    assert {c.k_bins for c in cases} == set(lc.BINS)
    for p in lc.ORDERS:
        assert {bool(c.pad) for c in cases if c.p == p} == {True, False}
    for c in cases:  # and the inputs are ordinary ones: every frame clean, every root found on the coarsest grid
        want = lc.reference(c)
        assert not want["bad"].any() and np.all(want["level"] == ref.G_MIN) and np.all(np.diff(want["x"], axis=1) < 0)


# ---- b. grid refinement ----------------------------------------------------------------------------------------------
def test_every_grid_level_occurs_on_the_device():
    """Predictors built from chosen frequencies: the reference needs level 256, 512, 1024 and 4096 and exhausts 4096 on
    the last — and so does the device, with the same bits, the flag for the last frame only."""
    rt = _rt()
    a, levels, _ = lc.refinement_predictors()
    x, level = lc.refinement_reference()
    assert level.tolist() == levels.tolist() == [256, 512, 1024, 4096, 0]
    got = lc.run_lsf(rt, a, pad=2)
    assert lc.compare(got, {"x": x, "level": level}, ("x", "level")) == []
    assert _lsf_flag(rt.take_flags()) == 1
    clean = lc.run_lsf(rt, a[:4])
    assert lc.compare(clean, {"x": x[:4], "level": level[:4]}, ("x", "level")) == []
    assert rt.take_flags() == [0] * 16


# ---- c. degenerate rows ----------------------------------------------------------------------------------------------
def test_degenerate_rows_touch_no_other_frame_and_raise_the_flag_exactly_then():
    rt = _rt()
    p = 24
    r, odd = lc.degenerate_rows(p)
    want = lc.stages(r, p, 129)
    flagged = sorted(i for i, kind in odd.items() if kind != "zero")
    assert np.nonzero(want["bad"])[0].tolist() == flagged and np.nonzero(want["level"] == 0)[0].tolist() == flagged
    got = lc.run_levinson(rt, r, p, pad=1)
    assert lc.compare(got, want, ("a", "e", "refl")) == []
    assert _lsf_flag(rt.take_flags()) == 1
    assert got["e"][3] == 0.0 and got["a"][3].tolist() == [1.0] + [0.0] * p and np.all(np.isnan(got["a"][flagged]))
    two = lc.run_lsf(rt, want["a"])
    assert lc.compare(two, want, ("x", "level")) == []
    assert _lsf_flag(rt.take_flags()) == 1
    three = lc.run_envelope(rt, want["ex"], 129)
    assert lc.compare(three, want, ("env",)) == []
    assert np.all(three["env"][3] == 0.0) and np.all(np.isnan(three["env"][flagged]))
    assert rt.take_flags() == [0] * 16  # (the envelope raises nothing: NaN rows flow through)
    # the clean rows alone: the same bits, and no flag; the all-zero row alone raises none either
    keep = np.array([i for i in range(len(r)) if i not in odd])
    alone = lc.run_levinson(rt, r[keep], p)
    assert lc.compare(alone, {k: want[k][keep] for k in ("a", "e", "refl")}, ("a", "e", "refl")) == []
    x_alone = lc.run_lsf(rt, want["a"][keep])
    assert lc.same_bits(x_alone["x"], want["x"][keep])
    assert lc.same_bits(lc.run_levinson(rt, r[3:4], p)["a"], want["a"][3:4])
    assert rt.take_flags() == [0] * 16
    # each kind of bad row on its own raises the flag
    for i in flagged:
        lc.run_levinson(rt, r[i:i + 1], p)
        assert _lsf_flag(rt.take_flags()) == 1, odd[i]


def test_the_same_call_twice_gives_the_same_bits():
    rt = _rt()
    case = next(c for c in lc.kernel_cases() if c.p == 40 and c.frames == 257)
    one, two = lc.run(rt, case), lc.run(rt, case)
    for key in lc.KEYS:
        assert lc.same_bits(one[key], two[key]), key


def test_an_empty_batch_is_no_error():
    from world.lsf import envelope_device, levinson_device, lsf_from_lpc_device

    rt = _rt()
    a, e, k = levinson_device(rt, rt.zeros((0, 25)), 24, want_reflection=True)
    assert tuple(a.shape) == (0, 25) and tuple(e.shape) == (0,) and tuple(k.shape) == (0, 24)
    assert tuple(lsf_from_lpc_device(rt, rt.zeros((0, 25))).shape) == (0, 24)
    assert tuple(envelope_device(rt, rt.zeros((0, 25)), 513).shape) == (0, 513)


# ---- d. the chain on the fixtures ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixtures():
    return {name: np.ascontiguousarray(np.load(os.path.join(GOLDEN, name + ".npz"))["ct_spectrogram"].T)
            for name in {t[0] for t in TABLE}}


@pytest.mark.parametrize("name,p,table_db", TABLE, ids=lambda v: str(v))
def test_chain_on_the_fixture(fixtures, name, p, table_db):
    """Autocorrelation within the product kernel's derived bound of the long-double product; the device's rows equal
    the reference run on the DEVICE's autocorrelation bit for bit (log and acos are the library's: compared in the cosine
    domain and as prediction errors); the distortion of the rebuilt envelope equals the reference's own within 1e-6 dB."""
    from world import lsf

    rt = _rt()
    spec = fixtures[name]
    k_bins = spec.shape[1]
    spec_d = rt.to_device(spec)
    r = lsf.autocorr_device(rt, spec_d, p).cpu().numpy()
    fr.check("autocorrelation %s p=%d" % (name, p), r, spec, k_bins, k_bins, None, 1.0, lsf.autocorr_table(k_bins, p).w, 0, 0)
    assert np.array_equal(lsf.autocorr_table(k_bins, p).w, ref.autocorr_table(k_bins, p))
    want = lc.stages(r, p, k_bins)
    a, e, refl = lsf.levinson_device(rt, rt.to_device(r), p, want_reflection=True)
    x, level = lsf.lsf_from_lpc_device(rt, a, want_level=True)
    got = {"a": a.cpu().numpy(), "e": e.cpu().numpy(), "refl": refl.cpu().numpy(), "x": x.cpu().numpy(),
           "level": level.cpu().numpy()}
    assert lc.compare(got, want, ("a", "e", "refl", "x", "level")) == []
    assert not want["bad"].any() and np.all(want["level"] > 0)
    # the public functions: rows in radians and back
    rows = lsf.lsf_device(rt, spec_d, p)
    assert tuple(rows.shape) == (spec.shape[0], p + 1)
    rows_h = rows.cpu().numpy()
    assert np.all(np.diff(rows_h[:, 1:], axis=1) > 0) and np.all(rows_h[:, 1] > 0) and np.all(rows_h[:, -1] < np.pi)
    assert np.allclose(rows_h[:, 1:], np.arccos(want["x"]), rtol=0, atol=8 * ref.U * np.pi)  # two acos of <= 2 ulp each
    assert np.allclose(rows_h[:, 0], np.log(want["e"]), rtol=0, atol=1e-13)
    env = lsf.ilsf_device(rt, rows, 2 * (k_bins - 1)).cpu().numpy()
    lsd_device = ref.lsd_db(env, spec)
    # the reference's own figure, from the spectrogram alone on the CPU
    rows_ref, _, bad = ref.lsf_rows(ref.autocorr(spec, p), p)
    lsd_ref = ref.lsd_db(ref.ilsf_rows(rows_ref, k_bins), spec)
    print("%s p=%d: LSD device %.9f dB, reference %.9f dB" % (name, p, lsd_device, lsd_ref))
    assert not bad.any() and abs(lsd_ref - table_db) < 5e-4
    assert abs(lsd_device - lsd_ref) <= 1e-6
    assert rt.take_flags() == [0] * 16


def _product_tolerance(w, k_bins):
    """Relative, per frame and bin: torch's cos and exp against NumPy's differ by at most 2 ulp each, so a factor
    2 c - 2 x_i differs by at most 8 u / |c - x_i| of itself; p factors, squared halves summed, and the gain."""
    x = np.cos(w)
    d = np.min(np.abs(ref.bin_table(k_bins)[None, :, None] - x[:, None, :]), axis=2)
    return 8 * w.shape[1] * ref.U / d + 64 * ref.U


def test_repair_makes_unsorted_rows_decodable():
    """min_gap: rows with swapped, coinciding and out-of-range angles decode to a finite positive envelope, equal to the
    reference's (the repair is torch's elementwise max / min / +: the same operations) within the rounding of cos / exp;
    without it they are used as they are."""
    from world import lsf

    rt = _rt()
    rng = np.random.RandomState(3)
    p, gap = 24, 1e-3
    w = np.sort(rng.uniform(0.05, 3.09, size=(40, p)), axis=1)
    w[1, 5], w[1, 6] = w[1, 6], w[1, 5]
    w[2, 10] = w[2, 11]
    w[3, 0], w[3, -1] = -0.2, 3.5
    w[4] = 1.0
    rows = np.concatenate([rng.randn(40, 1), w], axis=1)
    got = lsf.ilsf_device(rt, rt.to_device(rows), 1024, min_gap=gap).cpu().numpy()
    fixed = ref.repair(w, gap)
    assert np.all(np.diff(fixed, axis=1) >= gap * (1 - 1e-12)) and fixed.min() >= gap * (1 - 1e-12)
    want = ref.ilsf_rows(rows, 513, gap)
    assert np.all(np.isfinite(got)) and np.all(got > 0)
    assert np.all(np.abs(got - want) <= _product_tolerance(fixed, 513) * want)
    clean = np.array([i for i in range(40) if i not in (1, 2, 3, 4)])
    as_is = lsf.ilsf_device(rt, rt.to_device(rows[clean]), 1024).cpu().numpy()
    want = ref.ilsf_rows(rows[clean], 513)
    assert np.all(np.abs(as_is - want) <= _product_tolerance(w[clean], 513) * want)


def test_arguments_the_library_refuses():
    """Behind the Python checks: the C entries fail with a message, before anything is launched."""
    import ctypes

    from world.lsf import bin_table, grid_table

    rt = _rt()
    x, y = rt.zeros((4, 80)) + 1, rt.zeros((4, 600))
    dp = ctypes.POINTER(ctypes.c_double)
    grid, bins = grid_table(), bin_table(513)

    def lev(p=24, ldr=25, lda=25, ldk=24):
        return rt.lib.wh_lpc_levinson(rt.ctx, rt.stream(), rt.ptr(x), 4, ldr, p, rt.ptr(y), lda, rt.ptr(y[:, 100]), rt.ptr(y),
                                      ldk)

    def roots(p=24, lda=25, ldx=24, n_grid=4097):
        return rt.lib.wh_lsf_from_lpc(rt.ctx, rt.stream(), rt.ptr(x), 4, lda, p, grid.ctypes.data_as(dp), n_grid, rt.ptr(y),
                                      ldx, None)

    def env(p=24, ldr=25, k_bins=513, ldo=513):
        return rt.lib.wh_lsf_envelope(rt.ctx, rt.stream(), rt.ptr(x), 4, ldr, p, bins.ctypes.data_as(dp), k_bins, rt.ptr(y),
                                      ldo)

    for call, kw, word in ((lev, {"p": 0}, b"order"), (lev, {"p": 65}, b"order"), (lev, {"ldr": 24}, b"ldr"),
                           (lev, {"lda": 24}, b"lda"), (lev, {"ldk": 23}, b"ldk"),
                           (roots, {"p": 23}, b"even"), (roots, {"p": 66, "lda": 67, "ldx": 66}, b"order"),
                           (roots, {"p": 0}, b"order"), (roots, {"lda": 24}, b"lda"), (roots, {"ldx": 23}, b"ldx"),
                           (roots, {"n_grid": 4096}, b"4097"),
                           (env, {"p": 25, "ldr": 26}, b"even"), (env, {"ldr": 24}, b"ldr"), (env, {"k_bins": 1}, b"k_bins"),
                           (env, {"ldo": 512}, b"ldo")):
        assert call(**kw) != 0, kw
        assert word in rt.lib.wh_last_error(), (kw, rt.lib.wh_last_error())
    assert rt.lib.wh_lsf_envelope(None, None, None, 0, 25, 24, None, 513, None, 513) != 0
    assert lev() == 0 and roots() == 0 and env() == 0
    rt.torch.cuda.synchronize()
    rt.take_flags()
