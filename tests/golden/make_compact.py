"""Generate tests/golden/golden_compact.npz, the fixture of the band-aperiodicity expansion
(wh_aperiodicity_from_bands, world.compact), by running the UNMODIFIED reference.

Run only where the reference checkout that oracle/refshim.py points at exists:

    python tests/golden/make_compact.py

For a 1 s synthetic utterance at 16 kHz (one aperiodicity band) and one at 48 kHz (five bands: every segment of the
interpolation) it records what the reference's d4c() returns after dio -> stonemask -> cheaptrick:
  * `coarse_<tag>`  (nap, frames): 'coarse_ap', the negated band aperiodicity in dB (world/d4c.py:57,62);
  * `ap_<tag>`      (K, len(ap_frames)): the dense 'aperiodicity' (world/d4c.py:58-59) of the frames `ap_frames_<tag>`
    — every second one: the voiced rows are full-mantissa doubles that do not compress, and all 201 + 201 of them
    would make a file beyond the repository's 1 MiB limit for a committed file;
  * `failed_<tag>`  (frames,): `aperiodicity[0, :] > 0.5` — the frames the voicing gate rejected, whose rows hold
    1 - 1e-12 (world/d4c.py:49-51; bin 0 of every other frame is 10 ** (-60 / 20)).  The kernel's `gate` is its complement;
  * `fs_<tag>`, `fft_size_<tag>`.
Arrays only: no reference source text is stored."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import refshim  # noqa: E402

CASES = (("16k", 16000, 11), ("48k", 48000, 12))  # tag, rate, synthetic utterance


def main():
    R = refshim.load()
    spec = importlib.util.spec_from_file_location("_synthetic", os.path.join(ROOT, "python-world_amd", "world", "_synthetic.py"))
    syn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(syn)
    out = {}
    for tag, fs, u in CASES:
        x = syn.synth_utterance(u, fs, 1.0)
        d = R.dio.dio(x.copy(), fs)
        f0 = R.stonemask.stonemask(x, fs, d["temporal_positions"], d["f0"])
        src = {"f0": f0.copy(), "vuv": d["vuv"].copy(), "temporal_positions": d["temporal_positions"].copy()}
        R.cheaptrick.cheaptrick(x, fs, src)  # (writes its 500 Hz substitutions back into f0, as in World.encode)
        a = R.d4c.d4c(x, fs, src)
        ap = a["aperiodicity"]
        failed = ap[0, :] > 0.5
        assert failed.any() and (~failed).any(), tag
        out["fs_" + tag] = fs
        out["fft_size_" + tag] = (ap.shape[0] - 1) * 2
        out["coarse_" + tag] = a["coarse_ap"].copy()
        out["failed_" + tag] = failed
        cols = np.arange(0, ap.shape[1], 2)
        assert failed[cols].any() and (~failed[cols]).any(), tag
        out["ap_frames_" + tag] = cols
        out["ap_" + tag] = ap[:, cols].copy()
        print(tag, "coarse", a["coarse_ap"].shape, "aperiodicity", ap.shape, "gate-failed frames", int(failed.sum()))
    path = os.path.join(HERE, "golden_compact.npz")
    np.savez_compressed(path, **out)
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
