"""CPU: the long-double reference of tests/test_hip_fft_engine.py checked against the DFT sum itself, the restated radix
plan against the two plans csrc/wh_fft.h states in its comments, and a tripwire over the transforms' call sites."""
import glob
import os
import re

import numpy as np

import _fft_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python-world_amd", "csrc")


def _rel(got, ref):
    d2 = (got[0] - ref[0]) ** 2 + (got[1] - ref[1]) ** 2
    r2 = ref[0] ** 2 + ref[1] ** 2
    return float(np.sqrt(np.sum(d2) / np.sum(r2)))


def test_long_double_fft_against_the_direct_sum():
    for n in (64, 256):
        rng = np.random.RandomState(n)
        x = rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))
        for inverse in (False, True):
            err = _rel(R.fft(x, inverse), R.dft_direct(x, inverse))
            print("n = %d inverse = %d: fft against the direct long-double sum %.3g" % (n, inverse, err))
            assert err < 1e-17, (n, inverse, err)
        # the real wrappers: the half spectrum of the same sum, and back to n times the input
        xr = rng.standard_normal((3, n))
        full = R.dft_direct(xr)
        assert _rel(R.rfft(xr), (full[0][:, :n // 2 + 1], full[1][:, :n // 2 + 1])) < 1e-17
        back = R.irfft(*R.rfft(xr)) / n
        assert float(np.sqrt(np.sum((back - xr) ** 2) / np.sum(xr ** 2))) < 1e-17
    # and numpy's own double transform lies where a correct FP64 FFT should: a few 1e-16 from it
    x = np.random.RandomState(1).standard_normal((4, 8192)) + 0j
    f = np.fft.fft(x, axis=1)
    assert 5e-17 < _rel((f.real.astype(R.LD), f.imag.astype(R.LD)), R.fft(x)) < 5e-16


def test_twiddles_are_exact_on_the_axes_and_symmetric():
    for n in (2, 4, 8, 64, 4096):
        c, s = R.twiddles(n)
        assert c[0] == 1 and s[0] == 0 and c[n // 2] == -1 and s[n // 2] == 0
        if n >= 4:
            assert c[n // 4] == 0 and s[n // 4] == -1 and c[3 * n // 4] == 0 and s[3 * n // 4] == 1
        eps = np.finfo(R.LD).eps  # (cos and sin of pi/4 are two roundings of one number: conjugate pairs agree to an ulp)
        assert float(np.max(np.abs(c[1:] - c[1:][::-1]))) <= eps and float(np.max(np.abs(s[1:] + s[1:][::-1]))) <= eps
        assert float(np.max(np.abs(c * c + s * s - 1))) < 4 * np.finfo(R.LD).eps


def test_restated_radix_plan():
    assert R.plan(512, 64) == [8, 8, 8]            # wh_fft.h: "fft_lds<N, INV, GT> runs 8-8-8 (GT <= 128 at N = 512)"
    assert R.plan(512, 128) == [8, 8, 8]
    assert R.plan(512, 256) == [4, 4, 4, 4, 2]     # "a 256-thread group's 4-4-4-4-2 plan"
    assert R.plan(2048, 256) == [8, 8, 8, 4]       # "radix 8 needs 4 passes for 2048 points where radix 4 needs 6"
    assert R.plan(2048, 256, 4) == [4, 4, 4, 4, 4, 2]
    assert R.plan(8192, 512) == [8, 8, 8, 8, 2]
    assert R.plan(32, 32) == [4, 4, 2]
    assert R.passes(8192, 512, 4) == 7
    assert R.TWIDDLE_ENTRIES == 2 * 32768 + 8191 + 3 * 4095 + 7 * 2047


# (file, function) -> call sites in csrc/ (comments stripped; wh_fft.h itself, where the transforms are defined and call
# each other, and the probe are left out)
CALL_SITES = {
    ("wh_api.hip", "fft_lds_wave"): 2,
    ("wh_bands.h", "fft_lds"): 1,
    ("wh_bands.h", "rfft_lds"): 3,
    ("wh_cheaptrick.hip", "fft_lds"): 3,
    ("wh_cheaptrick.hip", "rfft_lds"): 1,
    ("wh_d4c.hip", "fft_lds"): 3,
    ("wh_d4c.hip", "fft_lds_from_regs"): 2,
    ("wh_d4c.hip", "rfft_lds"): 2,
    ("wh_minphase.h", "fft_lds"): 1,
    ("wh_minphase.h", "fft_lds_wave"): 2,
    ("wh_requiem.hip", "rfft_lds"): 1,
    ("wh_swipe.hip", "rfft_lds"): 1,
}


def test_call_site_tripwire():
    pat = re.compile(r"(?<![A-Za-z0-9_])(fft_lds_from_regs|fft_lds_wave|irfft_lds|rfft_lds|fft_lds)<")
    found = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))):
        name = os.path.basename(path)
        if name in ("wh_fft.h", "wh_fft_probe.hip"):
            continue
        with open(path) as f:
            text = f.read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        for m in pat.finditer(text):
            found[(name, m.group(1))] = found.get((name, m.group(1)), 0) + 1
    assert found == CALL_SITES, (
        "the call sites of the shared transforms have changed: %r now, %r in this test.  Add the new call site's "
        "(kind, N, NT, SNT, MAXR, direction) shapes to WH_PROBE_SHAPES in csrc/wh_fft_probe.hip and to SHAPES in "
        "tests/test_hip_fft_engine.py, then update CALL_SITES here"
        % (sorted(set(found.items()) - set(CALL_SITES.items())), sorted(set(CALL_SITES.items()) - set(found.items()))))


def test_the_probe_builds_the_shapes_the_gpu_test_lists():
    from test_hip_fft_engine import SHAPES

    with open(os.path.join(CSRC, "wh_fft_probe.hip")) as f:
        text = f.read()
    body = text[text.index("#define WH_PROBE_SHAPES(X)"):text.index('extern "C"')]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    built = []
    for m in re.finditer(r"(WH_PROBE_FWD_INV\(X,|X\()([^)]*)\)", body):
        v = [int(t) for t in m.group(2).split(",")]
        built += [(0,) + tuple(v) + (0,), (0,) + tuple(v) + (1,)] if m.group(1).startswith("WH_PROBE") else [tuple(v)]
    assert len(built) == len(set(built)) and set(built) == set(SHAPES), sorted(set(built) ^ set(SHAPES))
