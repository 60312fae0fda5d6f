"""Generate tests/golden/golden_timebase.npz by running the UNMODIFIED reference's time base on the case table of
tests/_timebase_cases.py.  Run only in the authoring container (needs the reference checkout, oracle/refshim.py):

    python tests/golden/make_timebase_golden.py [output.npz]

Per case the fixture holds what world/synthesis.py's time_base_generation returns (pulse times, 1-based indices,
fractional shifts, the per-sample voicing, bit-packed) and temporal_position_index as synthesis() derives it
(world/synthesis.py:50-52): recorded results only, no reference source text.
tests/test_timebase_reference_host.py compares tests/_timebase_reference.py with it, bit for bit."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import refshim  # noqa: E402

refshim.install()
import importlib  # noqa: E402

from scipy.interpolate import interp1d  # noqa: E402

ref_syn = importlib.import_module("world.synthesis")  # the reference's, first on sys.path after install()

import _timebase_cases as TC  # noqa: E402
import _timebase_reference as TR  # noqa: E402


def run(name, fs, tp, f0, vuv, out):
    t = np.arange(tp[0], tp[-1] + 1 / fs, 1 / fs)
    times, idx, shift, vuv_i = ref_syn.time_base_generation(tp, f0, fs, vuv, t, 500)
    tpi = interp1d(tp, np.arange(1, len(tp) + 1), fill_value='extrapolate')(times)
    tpi = np.maximum(1, np.minimum(len(tp), tpi))
    out[name + ".times"] = np.asarray(times, dtype=np.float64)
    out[name + ".pidx"] = np.asarray(idx, dtype=np.int64)
    out[name + ".shift"] = np.asarray(shift, dtype=np.float64)
    out[name + ".vuv_bits"] = np.packbits(np.asarray(vuv_i, dtype=bool))
    out[name + ".ny"] = np.int64(len(t))
    out[name + ".pos_idx"] = np.asarray(tpi, dtype=np.float64)


def main(path):
    out = {}
    for c in TC.cases():
        run(c.name, c.fs, c.tp, c.f0, c.vuv, out)
    for c in TC.fused_cases():
        run("fused." + c.name, c.fs, c.tp, TR.final_f0(c.f0, c.vuv, TR.low_limit(c.fs, c.fft_size)), c.vuv, out)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "golden_timebase.npz"))
