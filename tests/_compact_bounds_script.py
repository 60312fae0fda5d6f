"""Helper of tests/test_hip_compact_bounds.py: runs in a process whose WH_LIB is the bounds build (tests/_variants.py,
bounds: ap_from_bands_kernel and ap_gate_kernel of wh_apbands.hip index their global and LDS buffers through wh::ckp
there).  The inputs of tests/test_hip_compact.py's bitwise tests and of its end-to-end test."""
import os

import numpy as np

import _variants as V


def main():
    import torch

    from world import _hip, main as wmain
    from world._synthetic import synth_utterance
    from world.batch import WorldBatch
    from world.d4c import aperiodicity_from_bands_device

    wb = WorldBatch(0)
    rt = wb.rt
    rep = V.Report(rt)

    def case(name, xs, fs):
        enc = wb.encode(xs, fs, f0_method="dio", want_coarse=True)
        with rt.on_stream():
            back = aperiodicity_from_bands_device(rt, enc.coarse_ap, enc.ap_gate, fs, enc.fft_size)
        rep.case(name, frames=enc.batch.total_frames, equal=bool(torch.equal(back, enc.aperiodicity)))

    # the inputs of tests/test_hip_compact.py's bitwise tests
    for tag in ("syn16k", "syn48k"):
        g = np.load(os.path.join(V.HERE, "golden", "golden_%s.npz" % tag))
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
        rep.case("facade requiem=%s" % req, rt=_hip.Runtime.get(), frames=sum(len(d["f0"]) for d in dats),
                 equal=bool(all(np.isfinite(d["out"]).all() for d in dats)))
    rep.emit()


if __name__ == "__main__":
    main()
