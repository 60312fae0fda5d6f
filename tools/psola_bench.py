"""wh_psola (world/psola.py) at corpus sizes, on resident made recordings (tools/tsm_bench.py's: three
harmonics of a pitch gliding from 140 to 100 Hz plus a little noise) and period tracks made from that glide on the device:
64 and 1024 utterances of 10 s at 16 kHz and 16 of 60 s at 48 kHz, each at pitch 5/4, 4/5 and under a contour that rises
from 0.8 to 1.25 times the recording's f0, at the recording's own duration and psola.default_params(fs).

Per size and setting:
  marks_ms / smarks_ms / ola_ms   psola_marks_kernel (stage A), psola_smarks_kernel (B) and psola_ola_kernel (C) from the
                          library's per-launch event pairs;
  candidate_samples       the sum over the voiced analysis marks of P (2 D + 1), from the marks the call returned, and
                          ``share_of_fp64_vector_rate``: stage A's 4 FP64 operations per candidate sample (two products,
                          two sums, unfused) against the 39.3e12 FP64 vector instructions per second of the device;
  bytes_moved             what the three kernels read and write — per voiced mark the template and the candidate region
                          (2 P + 2 D doubles) and its 12-byte record; per grain the 29 bytes stage B writes and the 16 it
                          reads; per output sample two inputs and y — and a device copy_ of as many bytes beside it;
  psola_device_ms         psola_device (the raw call on tracks that are already made) between two events;
  tracks_ms / modify_ms   tracks_device and modify_device from a resident encoding of the batch (frame times every 5 ms,
                          the glide's f0, every frame voiced: a made BatchEncoding's three per-frame tensors and its frame
                          offsets): the three tracks built with torch operations, and tracks + wh_psola end to end.  What
                          modify_ms leaves out is the f0 analysis itself — the encoding is what the conversion pipeline
                          already holds —, which shift_pitch_device does not need;
  shift_pitch_ms          world.tsm.shift_pitch_device on the same batch at the same ratio (none for the contour);
  workgroups              one per utterance: what stages A and B can occupy of the device's 256 CUs.
``numpy_reference``: tests/_psola_reference.py on one host core for one second of one utterance, per setting.
Medians over --calls after --warmup.  Prints one JSON line and writes it to --out.

    python tools/psola_bench.py [--calls 5] [--warmup 1] [--sizes 64x10@16000,1024x10@16000,16x60@48000]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-world_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from tsm_bench import FP64_VECTOR_RATE, kernels_ms, made_recordings, med, timed  # noqa: E402

SETTINGS = ("5/4", "4/5", "contour")
NAMES = ("psola_marks_kernel", "psola_smarks_kernel", "psola_ola_kernel")


def made_tracks(rt, utts, n, fs, p, setting):
    """(per_a, per_s, src) of the made recordings: the glide's period on the grid, and the target's."""
    import torch

    k = torch.arange(n // p.grid + 1, device=rt.device, dtype=torch.float64) * p.grid
    f0 = 140.0 - 40.0 * k / n
    factor = {"5/4": torch.full_like(k, 1.25), "4/5": torch.full_like(k, 0.8), "contour": 0.8 + 0.45 * k / n}[setting]
    fs_t = torch.full_like(k, float(fs))
    per_a = torch.floor(fs_t / f0 + 0.5).to(torch.int32)
    per_s = torch.floor(fs_t / (f0 * factor) + 0.5).to(torch.int32)
    return per_a.repeat(utts), per_s.repeat(utts), k.to(torch.int64).repeat(utts)


class MadeEncoding:
    """What world.psola reads of an encoding: frame offsets, frame times, f0 and vuv — 5 ms frames, the glide's f0, voiced."""

    def __init__(self, rt, utts, n, fs):
        import torch

        frames = int(n / (fs * 0.005)) + 1
        tp = torch.arange(frames, device=rt.device, dtype=torch.float64) * 0.005
        self.frame_off = np.arange(utts + 1, dtype=np.int64) * frames
        self.temporal_positions = tp.repeat(utts)
        self.f0 = (140.0 - 40.0 * tp * fs / n).repeat(utts)
        self.vuv = torch.ones_like(self.f0)


def size_case(rt, utts, seconds, fs, calls, warmup):
    import torch

    import _psola_reference as pref
    from world import psola, tsm

    p = psola.default_params(fs)
    n = int(seconds * fs)
    x_off = np.arange(utts + 1, dtype=np.int64) * n
    x = made_recordings(rt, utts, n, fs)
    enc = MadeEncoding(rt, utts, n, fs)
    case = {"utterances": utts, "seconds": seconds, "fs": fs, "params": list(p), "workgroups": utts, "settings": {}}

    def copy_ms(nbytes):
        src = torch.zeros((nbytes // 16,), device=rt.device, dtype=torch.float64)
        dst = torch.empty_like(src)
        ms = timed(lambda: dst.copy_(src), calls, warmup)
        del src, dst
        torch.cuda.empty_cache()
        return ms

    for setting in SETTINGS:
        per_a, per_s, src = made_tracks(rt, utts, n, fs, p, setting)
        run = lambda: psola.psola_device(rt, x, x_off, [n] * utts, per_a, per_s, src, p)  # noqa: E731
        ms = kernels_ms(rt, NAMES, run, calls, warmup)
        device_ms = timed(run, calls, warmup)
        if setting == "contour":
            kw = {"f0": enc.f0 * (0.8 + 0.45 * enc.temporal_positions * fs / n)}
        else:
            kw = {"pitch": {"5/4": 1.25, "4/5": 0.8}[setting]}
        tracks_ms = timed(lambda: psola.tracks_device(rt, x_off, fs, enc, **kw), calls, warmup)
        modify_ms = timed(lambda: psola.modify_device(rt, x, x_off, fs, enc, **kw), calls, warmup)
        _, _, m = psola.psola_device(rt, x, x_off, [n] * utts, per_a, per_s, src, p, want_marks=True)
        n_marks, n_smarks = int(m["n_marks"].sum().item()), int(m["n_smarks"].sum().item())
        cap = psola.mark_capacity(n, p)
        per = m["periods"][:cap][:int(m["n_marks"][0].item())].cpu().numpy().astype(np.int64)  # (every utterance has the same)
        voiced = per[:-1][per[:-1] > 0]
        d = np.minimum(p.tol, voiced // 4)
        cand = int(np.sum(voiced * (2 * d + 1))) * utts
        b = utts * int(np.sum(8 * (2 * voiced + 2 * d) + 12)) + n_smarks * (29 + 16) + utts * n * (16 + 8)
        cp = copy_ms(b)
        total = sum(ms.values())
        out = {"output_samples": utts * n, "marks": n_marks, "grains": n_smarks, "marks_ms": ms[NAMES[0]], "smarks_ms": ms[NAMES[1]],
               "ola_ms": ms[NAMES[2]], "kernels_ms": total, "psola_device_ms": device_ms, "tracks_ms": tracks_ms,
               "modify_ms": modify_ms, "candidate_samples": cand,
               "candidate_samples_per_s": cand / (ms[NAMES[0]] * 1e-3),
               "share_of_fp64_vector_rate": 4 * cand / (ms[NAMES[0]] * 1e-3) / FP64_VECTOR_RATE,
               "us_per_mark_per_workgroup": 1e3 * ms[NAMES[0]] / max(len(per), 1),
               "us_per_grain_per_wave": 1e3 * ms[NAMES[1]] / max(n_smarks // utts, 1),
               "bytes_moved": b, "gb_per_s": b / total / 1e6, "copy_same_bytes_ms": cp, "over_copy": total / cp}
        if setting != "contour":
            num, den = (int(v) for v in setting.split("/"))
            out["shift_pitch_ms"] = timed(lambda: tsm.shift_pitch_device(rt, x, x_off, fs, num / den), calls, warmup)
        x1 = x[:fs].cpu().numpy()
        k1 = fs // p.grid + 1
        t0 = time.perf_counter()
        pref.psola(x1, fs, per_a[:k1].cpu().numpy(), per_s[:k1].cpu().numpy(), src[:k1].cpu().numpy(), pref.Params(*p))
        ref_s = time.perf_counter() - t0
        out["numpy_reference_s_per_utterance_second"] = ref_s
        out["numpy_reference_one_core_s_extrapolated"] = ref_s * utts * seconds
        case["settings"][setting] = out
        del m, per_a, per_s, src
    del x
    torch.cuda.empty_cache()
    rt.trim()
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="64x10@16000,1024x10@16000,16x60@48000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_psola_bench.json"))
    a = ap.parse_args()
    from world import _hip

    rt = _hip.Runtime.get()
    out = {"calls": a.calls, "warmup": a.warmup, "fp64_vector_instructions_per_s": FP64_VECTOR_RATE, "sizes": {}}
    for s in a.sizes.split(","):
        shape, fs = s.split("@")
        utts, seconds = shape.split("x")
        out["sizes"][s] = size_case(rt, int(utts), float(seconds), int(fs), a.calls, a.warmup)
    assert rt.take_flags() == [0] * 16
    line = json.dumps(out)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
