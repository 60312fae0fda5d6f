"""GPU: the BOUNDS build.  The image cannot run device AddressSanitizer, and round 5's attempt left
an abort of the instrumented cheaptrick_kernel<1024> that could not be read.  The deterministic replacement is a build of
the library in which the covered kernels index every buffer through checked pointers (csrc/wh_device.h, wh::ckp: T* in
the shipped build, a range-carrying pointer under -DWH_BOUNDS=1): an access outside a named buffer is recorded (buffer,
index, size), reported as WH_FLAG_OOB by wh_take_flags and redirected, so the run completes and says what happened.
Covered: cheaptrick_kernel (LDS buffers, waveform gather, twiddle table, output rows), wh_spectral.h (low-band replica,
mirrored fill, sliding band windows), every transform helper (fft_lds / rfft_lds / irfft_lds and their passes), the block
reductions, and — the kernels the sanitizer could not load — stonemask_tab_kernel, hv_refine_kernel and the exact phase
scan.  The test builds that variant (hipcc, ~1 min) if it is not there, runs tests/_bounds_script.py against it and
expects: the positive control fires with the right record; the CheapTrick fixtures reproduce the reference with zero
records; an f0 sweep from 1 Hz to 1.5 fs at five (rate, transform) pairs — caller-supplied contours the reference's
estimators never return (world/cheaptrick.py:64-131 takes any f0) — stays inside every buffer; config 2 at its full
size, a Harvest + Requiem batch and a 48 kHz utterance run clean; the transform probe (csrc/wh_fft_probe.hip), one launch
each of a handful of shapes, stays inside its LDS buffers and the twiddle block; the selection probe and the two spectral
probes (csrc/wh_d4c_probe.hip, csrc/wh_spectral_probe.hip), one call per shape on the inputs that reach furthest — every selection
round and refinement level, the replica with every bin a node — stay inside theirs."""
import pytest

import _variants as V

pytestmark = pytest.mark.gpu

report = V.report_fixture("bounds", "_bounds_script.py", timeout=900)


def test_the_checker_fires_on_the_positive_control(report):
    assert report["bounds_build"] is True
    assert report["selftest_flag"] == 1
    assert report["selftest_record"] == [1, 7, 4, 4]  # one access, WH_CK_TABLE, element 4 of 4
    assert report["clean_after"] == [0, [0, 0, 0, 0]]  # read-and-clear


def test_cheaptrick_fixtures_run_inside_their_buffers(report):
    for tag, r in report["fixtures"].items():
        assert r["flag"] == 0 and r["record"] == [0, 0, 0, 0], (tag, r)
        assert r["rel_rms"] < 1e-9, (tag, r)  # and reproduce the reference (tests/test_hip_cheaptrick.py's bar)


def test_cheaptrick_f0_sweep_stays_inside_its_buffers(report):
    assert report["sweep_cases"] == 75
    assert report["sweep_bad"] == []


def test_d4c_f0_sweep_stays_inside_its_buffers(report):
    assert report["d4c_sweep_cases"] == 135
    assert report["d4c_sweep_bad"] == []


def test_decode_sweep_stays_inside_its_buffers(report):
    assert report["decode_sweep_cases"] == 60
    assert report["decode_sweep_flags"] == [0] * 16, (report["decode_sweep_flags"], report["decode_sweep_record"])


def test_off_regime_signals_run_clean(report):
    assert report["fuzz_flags"] == [0] * 16, (report["fuzz_flags"], report["fuzz_record"])


def test_whole_pipelines_run_clean(report):
    for key in ("config2", "harvest", "cfg5"):
        assert report[key + "_flags"] == [0] * 16, (key, report[key + "_flags"], report[key + "_record"])


def test_transform_probe_stays_inside_its_buffers(report):
    # 64 points on one wave, two chains in lockstep, the 128 KB transform, the register-fed first pass, rfft_lds on 64 threads,
    # irfft_lds; 37 transforms each (a half-filled last workgroup where two share one)
    assert len(report["fft_probe"]) == 6
    for shape, r in report["fft_probe"].items():
        assert r["rc"] == 0 and r["flag"] == 0 and r["record"] == [0, 0, 0, 0] and r["finite"], (shape, r)


def test_selection_probe_stays_inside_its_buffers(report):
    # sum_smallest at d4c_kernel's five shapes, both assignments: ten selection rounds, and every refinement level with the
    # whole row in the ranked list
    assert len(report["select_probe"]) == 10
    for shape, r in report["select_probe"].items():
        assert r["rc"] == 0 and r["flag"] == 0 and r["record"] == [0, 0, 0, 0] and r["finite"], (shape, r)


def test_spectral_probes_stay_inside_their_buffers(report):
    # the replica with every bin a node (f0 around fs / 2: the mirror branch of the LDS form, several waves of the runs
    # form) and the smoothing, both forms at every shape
    assert len(report["spectral_probes"]) == 20
    for shape, r in report["spectral_probes"].items():
        assert r["rc"] == 0 and r["flag"] == 0 and r["record"] == [0, 0, 0, 0] and r["finite"], (shape, r)


def test_shipped_library_is_not_a_bounds_build():
    from world import _hip

    assert _hip.bounds_build() is False
    rt = _hip.Runtime.get()
    with pytest.raises(_hip.WorldHipError):
        _hip.check(rt.lib.wh_bounds_selftest(rt.ctx, rt.stream()))
