"""CPU: the NumPy reference of the time base (tests/_timebase_reference.py) and the case table of the GPU test
(tests/_timebase_cases.py), pinned without a GPU:
  * against oracle.resynth.synthesis_np's aux outputs on the golden fixtures and on every case;
  * against the UNMODIFIED reference's time_base_generation, recorded in tests/golden/golden_timebase.npz
    (tests/golden/make_timebase_golden.py), and — where the reference checkout is present, i.e. in the authoring
    container — against a fresh run of it;
  * the conditions on the table: no case makes the reference raise or index outside 1 <= idx <= ny - 1, frame times
    start within [0, 3 / fs], and every case shows the property it exists for on the reference alone."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _timebase_cases as TC
import _timebase_reference as TR
from conftest import GOLDEN
from oracle import refshim, resynth


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


_refs = {}


def ref_of(case):
    if case.name not in _refs:
        _refs[case.name] = TR.timebase_np(case.tp, case.f0, case.vuv, case.fs)
    return _refs[case.name]


def _against_synthesis_np(tp, f0, vuv, fs, r):
    k = 3  # (the spectra do not enter the quantities compared: the smallest transform synthesis_np takes)
    spec = np.ones((k, len(tp)))
    ap = np.full((k, len(tp)), 0.5)
    _, aux = resynth.synthesis_np(f0, vuv, tp, spec, ap, fs, noise=np.zeros(r["draws"]), return_aux=True)
    assert np.array_equal(aux["pulse_index"], r["pidx"])
    assert np.array_equal(_bits(aux["pulse_shift"]), _bits(r["shift"]))
    assert np.array_equal(_bits(aux["pulse_times"]), _bits(r["time"]))
    assert aux["noise_used"] == r["draws"] == int(r["noff"][-1]) + max(3, int(r["noise_size"][-1]))


@pytest.mark.parametrize("tag", ["syn16k", "syn48k"])
def test_reference_vs_synthesis_np_on_the_golden_fixtures(golden, tag):
    g = golden(tag)
    tp, f0, vuv, fs = g["tp"], g["d4c_f0_after"], g["dio_vuv"], int(g["fs"])
    r = TR.timebase_np(tp, f0, vuv, fs)
    _, aux = resynth.synthesis_np(f0, vuv, tp, g["ct_spectrogram"], g["d4c_aperiodicity"], fs,
                                  noise=np.zeros(r["draws"]), return_aux=True)
    assert np.array_equal(aux["pulse_index"], r["pidx"])
    assert np.array_equal(_bits(aux["pulse_shift"]), _bits(r["shift"]))
    assert np.array_equal(_bits(aux["pulse_times"]), _bits(r["time"]))
    assert aux["noise_used"] == r["draws"]
    assert r["ny"] == len(g["syn_y"])


@pytest.mark.parametrize("name", TC.names())
def test_case_conditions_hold_on_the_reference_alone(name):
    c = TC.by_name(name)
    assert 0.0 <= c.tp[0] <= 3.0 / c.fs and np.all(np.diff(c.tp) > 0)
    assert len(c.tp) == len(c.f0) == len(c.vuv) >= 2
    r = ref_of(c)  # raises NoPulse / IndexError where the reference would assert or index outside its phase
    assert r["count"] >= 1 and r["pidx"].min() >= 1 and r["pidx"].max() <= r["ny"] - 1
    assert np.all(np.diff(r["pidx"]) >= 0) and r["noise_size"][-1] == 0
    assert 0 <= r["row_lo"].min() and r["row_hi"].max() <= len(c.tp) - 1 and np.all(r["row_hi"] - r["row_lo"] <= 1)
    assert bool(c.holds(r)), c.why
    if name != "long_tile_parallel":
        assert r["ny"] <= 64 * 4096  # the others take the one-workgroup scan
    _against_synthesis_np(c.tp, c.f0, c.vuv, c.fs, r)


def test_case_table_covers_what_it_is_for():
    refs = [ref_of(c) for c in TC.cases()]
    assert len({c.name for c in TC.cases()}) == len(TC.cases())
    assert {c.fs for c in TC.cases()} >= {8000, 16000, 44100, 48000}
    assert any(r["same"].any() for r in refs) and any((~r["same"]).any() for r in refs)         # both weight branches
    assert any(np.any(r["b"] == 0.0) for r in refs) or any(np.any(r["b"] == 1.0) for r in refs)  # a weight at its end
    assert any(r["noise_size"][:-1].min() < 3 for r in refs)                                     # max(3, .) bites
    assert any(r["at"][-1] == r["ny"] - 2 for r in refs)                                         # the last pair
    assert sum(int(np.sum(r["at"] % 1024 == 1023)) for r in refs) >= 17 * 4                      # the tile seam
    assert any(np.any(r["at"] % 1024 == 0) for r in refs)
    assert sum(r["ny"] > 64 * 4096 for r in refs) == 1


@pytest.mark.parametrize("name", [c.name for c in TC.fused_cases()])
def test_fused_cases(name):
    c = {c.name: c for c in TC.fused_cases()}[name]
    lim = TR.low_limit(c.fs, c.fft_size)
    fin = TR.final_f0(c.f0, c.vuv, lim)
    assert np.all(fin[c.vuv == 0] == 0) and np.all(fin[(c.vuv != 0) & (c.f0 < lim)] == 500.0)
    assert np.array_equal(fin[(c.vuv != 0) & (c.f0 >= lim)], c.f0[(c.vuv != 0) & (c.f0 >= lim)])
    assert bool(c.holds(c.f0, c.vuv, fin)), c.why
    r = TR.timebase_np(c.tp, fin, c.vuv, c.fs)
    assert r["count"] >= 1
    _against_synthesis_np(c.tp, fin, c.vuv, c.fs, r)


def test_no_pulse_case_is_one_the_reference_asserts_on():
    c = TC.NO_PULSE
    assert len(np.arange(c.tp[0], c.tp[-1] + 1 / c.fs, 1 / c.fs)) == 17
    with pytest.raises(TR.NoPulse):
        TR.timebase_np(c.tp, c.f0, c.vuv, c.fs)
    with pytest.raises(AssertionError):
        resynth.pulse_train(c.tp, c.f0, c.fs, c.vuv)


def _compare_with_recorded(z):
    todo = [(c.name, c, None) for c in TC.cases()] + [("fused." + c.name, c, c.fft_size) for c in TC.fused_cases()]
    assert {k.rsplit(".", 1)[0] for k in z} == {n for n, _, _ in todo}
    for name, c, fft in todo:
        f0 = c.f0 if fft is None else TR.final_f0(c.f0, c.vuv, TR.low_limit(c.fs, fft))
        r = TR.timebase_np(c.tp, f0, c.vuv, c.fs) if fft is not None else ref_of(c)
        assert int(z[name + ".ny"]) == r["ny"], name
        assert np.array_equal(z[name + ".pidx"], r["pidx"]), name
        assert np.array_equal(_bits(z[name + ".times"]), _bits(r["time"])), name
        assert np.array_equal(_bits(z[name + ".shift"]), _bits(r["shift"])), name
        assert np.array_equal(_bits(z[name + ".pos_idx"]), _bits(r["pos_idx"])), name
        assert np.array_equal(np.unpackbits(z[name + ".vuv_bits"])[:r["ny"]], r["vuv_s"]), name


def test_reference_module_equals_the_recorded_reference():
    _compare_with_recorded(dict(np.load(os.path.join(GOLDEN, "golden_timebase.npz"))))


def test_recorded_reference_is_reproduced_where_the_reference_is_present(tmp_path):
    """In the authoring container the fixture is generated again from the unmodified reference and compared; anywhere
    else there is nothing to run and the committed fixture (above) is the pin."""
    if not os.path.isdir(os.path.join(refshim.REFERENCE_ROOT, "world")):
        return
    out = str(tmp_path / "tb.npz")
    subprocess.run([sys.executable, os.path.join(GOLDEN, "make_timebase_golden.py"), out], check=True,
                   stdout=subprocess.DEVNULL, timeout=300)
    fresh = dict(np.load(out))
    rec = dict(np.load(os.path.join(GOLDEN, "golden_timebase.npz")))
    assert set(fresh) == set(rec)
    for k in rec:
        assert fresh[k].dtype == rec[k].dtype and np.array_equal(fresh[k].view(np.uint8) if fresh[k].ndim else fresh[k],
                                                                 rec[k].view(np.uint8) if rec[k].ndim else rec[k]), k
