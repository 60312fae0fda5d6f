"""Helper of tests/test_hip_compact_bounds.py: runs in a process whose WH_LIB is the bounds build
(tools/build_variants.py bounds=...;wh_apbands:-DWH_BOUNDS=1: ap_from_bands_kernel and ap_gate_kernel index their global and
LDS buffers through wh::ckp there).  Prints one JSON line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "python-world_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import torch

    from world import _hip, main as wmain
    from world._synthetic import synth_utterance
    from world.batch import WorldBatch
    from world.d4c import aperiodicity_from_bands_device

    out = {"bounds_build": _hip.bounds_build(), "cases": []}
    wb = WorldBatch(0)
    rt = wb.rt

    def case(name, xs, fs):
        enc = wb.encode(xs, fs, f0_method="dio", want_coarse=True)
        with rt.on_stream():
            back = aperiodicity_from_bands_device(rt, enc.coarse_ap, enc.ap_gate, fs, enc.fft_size)
        eq = bool(torch.equal(back, enc.aperiodicity))
        fl = rt.take_flags()
        out["cases"].append({"name": name, "frames": enc.batch.total_frames, "equal": eq, "flag": fl[_hip.FLAG_OOB],
                             "flags": fl, "record": list(_hip.bounds_last())})

    # the inputs of tests/test_hip_compact.py's bitwise tests
    gold = os.path.join(ROOT, "tests", "golden")
    for tag in ("syn16k", "syn48k"):
        g = np.load(os.path.join(gold, "golden_%s.npz" % tag))
        case(tag, [g["x"]], int(g["fs"]))
    fs = 16000
    rng = np.random.RandomState(12)
    n = int(1.13 * fs)
    t = np.arange(n) / fs
    low = sum(np.sin(2 * np.pi * 140.0 * h * t + 0.3 * h) / h for h in range(1, 25))
    spec = np.fft.rfft(rng.randn(n))
    fr = np.fft.rfftfreq(n, 1 / fs)
    spec[(fr < 4300) | (fr > 7600)] = 0.0
    high = np.fft.irfft(spec, n)
    high *= np.sqrt(np.mean(low ** 2) / np.mean(high ** 2))
    case("ragged", [synth_utterance(21, fs, 0.7), np.zeros(int(0.31 * fs)),
                    0.2 * (low + np.linspace(0.15, 0.75, n) * high)], fs)
    # ... and of its end-to-end test, through the facade
    xs = [synth_utterance(31, fs, 0.8), synth_utterance(32, fs, 0.45), synth_utterance(33, fs, 1.1)]
    W = wmain.World()
    for req in (False, True):
        dats = W.decode_compact_batch(W.encode_compact_batch(fs, xs, n0=40, is_requiem=req), seed=7)
        fl = _hip.Runtime.get().take_flags()
        out["cases"].append({"name": "facade requiem=%s" % req, "frames": sum(len(d["f0"]) for d in dats),
                             "equal": bool(all(np.isfinite(d["out"]).all() for d in dats)), "flag": fl[_hip.FLAG_OOB],
                             "flags": fl, "record": list(_hip.bounds_last())})
    print("BOUNDS_JSON " + json.dumps(out))


if __name__ == "__main__":
    main()
