"""Generate tests/golden/golden_harvest_contour.npz by running the UNMODIFIED reference's RemoveUnreliableCandidates,
FixF0Contour and SmoothF0 (world/harvest.py:215-234, 301-404, 533-559) on the crafted candidate maps of
tests/_harvest_contour_cases.py.  Run only in the authoring container (needs the reference checkout, oracle/refshim.py):

    python tests/golden/make_harvest_contour_golden.py [output.npz]

Per case the fixture holds the pruned map (sparse: rows, frames, frequencies, scores of the surviving candidates), the
1 ms contour FixF0Contour returns, its vuv (bit-packed) and SmoothF0's output; per row of smooth_rows() SmoothF0's output.
Recorded results only, no reference source text.

MergeF0 orders the sections' extended starts with np.argsort(kind='quicksort'), which NumPy does not promise to be stable;
the kernels and the oracle order them stably.  For the cases with tied starts (TIED) the reference is run a second time
with a stable sort in its place, and `<case>.binding` records whether both runs gave the same contour here: where they
did, the fixture binds tests/test_harvest_contour_reference_host.py and the GPU test like any other."""
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

ref_hv = importlib.import_module("world.harvest")  # the reference's, first on sys.path after install()

import _harvest_contour_cases as HC  # noqa: E402


def contour(pc, ps, stable):
    """FixF0Contour, optionally with every argsort made stable"""
    plain = np.argsort
    if stable:
        np.argsort = lambda a, *args, **kw: plain(a, *args, **dict(kw, kind="stable"))
    try:
        return ref_hv.FixF0Contour(pc, ps)
    finally:
        np.argsort = plain


def main(path):
    out = {}
    for c in HC.cases():
        pc, ps = ref_hv.RemoveUnreliableCandidates(c.cands, c.scores)
        f0, vuv = contour(pc, ps, False)
        rows, frames = np.nonzero(pc)
        out[c.name + ".rows"] = rows.astype(np.uint8)
        out[c.name + ".frames"] = frames.astype(np.int32)
        out[c.name + ".f0"] = pc[rows, frames]
        out[c.name + ".score"] = ps[rows, frames]
        out[c.name + ".contour"] = np.asarray(f0, dtype=np.float64)
        out[c.name + ".vuv_bits"] = np.packbits(np.asarray(vuv) != 0)
        out[c.name + ".smoothed"] = np.asarray(ref_hv.SmoothF0(f0), dtype=np.float64)
        if c.name in HC.TIED:
            f0_stable, _ = contour(pc, ps, True)
            out[c.name + ".binding"] = np.bool_(np.array_equal(f0, f0_stable))
            print(c.name, "tied starts: the reference's own order gives", "the stable order's contour" if
                  out[c.name + ".binding"] else "ANOTHER contour (not binding)")
    for name, row in HC.smooth_rows().items():
        out["smooth." + name] = np.asarray(ref_hv.SmoothF0(row), dtype=np.float64)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "golden_harvest_contour.npz"))
