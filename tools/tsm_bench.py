"""wh_wsola (world/tsm.py) at corpus sizes, on resident made recordings (three harmonics of a gliding pitch
plus a little noise): 64 and 1024 utterances of 10 s at 16 kHz (H = 128, D = 80) and 16 of 60 s at 48 kHz (H = 384,
D = 240), each stretched by 5/4 and by 4/5.

Per size and ratio:
  search_ms / ola_ms      wsola_search_kernel and wsola_ola_kernel from the library's per-launch event pairs;
  candidate_samples_per_s frames x (2 D + 1) x (2 H - 1) per second of the search kernel, and ``share_of_fp64_vector_rate``:
                          its 4 FP64 operations per candidate sample (two products, two sums, unfused) against the 39.3e12
                          FP64 vector instructions per second of the device (256 CUs x 64 lanes x 2.4 GHz);
  bytes_moved             what the two kernels read and write — per frame the template and the candidate region
                          (4 H - 2 + 2 D doubles), its position, start and shift; per output sample two inputs, y — and
                          a device copy_ of as many bytes beside it;
  shift_pitch_ms          shift_pitch_device end to end between two events: the stretch, resample_device by the inverse
                          ratio and the trim into x's layout;
  workgroups              one per utterance: what the search kernel can occupy of the device's 256 CUs.
``numpy_reference``: tests/_wsola_reference.py on one host core for one second of one utterance, per ratio.
Medians over --calls after --warmup.  Prints one JSON line.

    python tools/tsm_bench.py [--calls 3] [--warmup 1] [--sizes 64x10@16000,1024x10@16000,16x60@48000]"""
import argparse
import json
import os
import sys
import time
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-world_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

FP64_VECTOR_RATE = 256 * 64 * 2.4e9  # FP64 vector instructions per second: a product or a sum each take one
RATIOS = (Fraction(5, 4), Fraction(4, 5))


def med(v):
    return float(np.median(v))


def timed(fn, calls, warmup):
    import torch

    out = []
    for i in range(warmup + calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            out.append(e0.elapsed_time(e1))
    return med(out)


def kernels_ms(rt, names, fn, calls, warmup):
    """{name: median ms} of the records whose name is in ``names`` over calls of fn()."""
    import torch

    out = {n: [] for n in names}
    for i in range(warmup + calls):
        if i == warmup:
            torch.cuda.synchronize()
            rt.profile(True)
        fn()
        if i >= warmup:
            rec = rt.profile_collect()
            for n in names:
                out[n].append(sum(ms for nm, ms in rec if nm == n))
    rt.profile(False)
    return {n: med(v) for n, v in out.items()}


def made_recordings(rt, utts, n, fs):
    """[utts * n]: per utterance three harmonics of a pitch gliding from 140 Hz to 100 Hz, with 1 % of noise."""
    import torch

    g = torch.Generator(device=rt.device).manual_seed(7)
    t = torch.arange(n, device=rt.device, dtype=torch.float64)
    phase = 2 * np.pi * torch.cumsum((140.0 - 40.0 * t / n) / fs, dim=0)
    one = torch.sin(phase) + 0.5 * torch.sin(2 * phase + 1.0) + 0.25 * torch.sin(3 * phase + 2.0)
    x = one.repeat(utts)
    x += 0.01 * torch.randn((utts * n,), generator=g, device=rt.device, dtype=torch.float64)
    return x


def size_case(rt, utts, seconds, fs, calls, warmup):
    import torch

    import _wsola_reference as wref
    from world import tsm

    hop, tol = tsm.default_hop_tol(fs)
    n = int(seconds * fs)
    x_off = np.arange(utts + 1, dtype=np.int64) * n
    x = made_recordings(rt, utts, n, fs)
    names = ("wsola_search_kernel", "wsola_ola_kernel")
    case = {"utterances": utts, "seconds": seconds, "fs": fs, "hop": hop, "tol": tol, "workgroups": utts, "ratios": {}}

    def copy_ms(nbytes):
        src = torch.zeros((nbytes // 16,), device=rt.device, dtype=torch.float64)
        dst = torch.empty_like(src)
        ms = timed(lambda: dst.copy_(src), calls, warmup)
        del src, dst
        torch.cuda.empty_cache()
        return ms

    for frac in RATIOS:
        n_out = tsm.stretched_length(n, frac)
        pos = [tsm.positions(n_out, hop, frac)] * utts
        frames = utts * len(pos[0])
        ms = kernels_ms(rt, names, lambda: tsm.wsola_device(rt, x, x_off, [n_out] * utts, pos, hop, tol), calls, warmup)
        _, _, delta = tsm.wsola_device(rt, x, x_off, [n_out] * utts, pos, hop, tol)
        cand_samples = frames * (2 * tol + 1) * (2 * hop - 1)
        b = frames * (8 * (4 * hop - 2 + 2 * tol) + 8 + 8 + 4) + utts * n_out * (16 + 8 + 8)
        cp = copy_ms(b)
        both = ms[names[0]] + ms[names[1]]
        end_to_end = timed(lambda: tsm.shift_pitch_device(rt, x, x_off, fs, frac), calls, warmup)
        x1 = x[:fs].cpu().numpy()
        n1 = tsm.stretched_length(len(x1), frac)
        t0 = time.perf_counter()
        wref.wsola(x1, n1, wref.positions(n1, hop, frac), hop, tol)
        ref_s = time.perf_counter() - t0
        case["ratios"]["%d/%d" % (frac.numerator, frac.denominator)] = {
            "output_samples": utts * n_out, "frames": frames, "search_ms": ms[names[0]], "ola_ms": ms[names[1]],
            "candidate_samples": cand_samples, "candidate_samples_per_s": cand_samples / (ms[names[0]] * 1e-3),
            "share_of_fp64_vector_rate": 4 * cand_samples / (ms[names[0]] * 1e-3) / FP64_VECTOR_RATE,
            "us_per_frame_per_workgroup": 1e3 * ms[names[0]] / len(pos[0]),
            "bytes_moved": b, "gb_per_s": b / both / 1e6, "copy_same_bytes_ms": cp, "over_copy": both / cp,
            "shift_pitch_ms": end_to_end, "mean_abs_shift": float(delta.abs().double().mean()),
            "numpy_reference_s_per_utterance_second": ref_s,
            "numpy_reference_one_core_s_extrapolated": ref_s * utts * seconds}
        del delta
    del x
    torch.cuda.empty_cache()
    rt.trim()
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="64x10@16000,1024x10@16000,16x60@48000")
    a = ap.parse_args()
    from world import _hip

    rt = _hip.Runtime.get()
    out = {"calls": a.calls, "warmup": a.warmup, "fp64_vector_instructions_per_s": FP64_VECTOR_RATE, "sizes": {}}
    for s in a.sizes.split(","):
        shape, fs = s.split("@")
        utts, seconds = shape.split("x")
        out["sizes"][s] = size_case(rt, int(utts), float(seconds), int(fs), a.calls, a.warmup)
    assert rt.take_flags() == [0] * 16
    print(json.dumps(out))


if __name__ == "__main__":
    main()
