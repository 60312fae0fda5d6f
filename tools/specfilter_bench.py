"""wh_spectral_filter (world/specfilter.py) at corpus sizes, on resident made tensors: 64 and 1024 utterances
of 10 s at 16 kHz (N = 1024, hop 80) and 16 of 60 s at 48 kHz (N = 2048, hop 240), gain rows on the 5 ms grid.

Per size, for kind 'lsf' (p = 40, numerator and denominator rows) and kind 'spectrum' (two [F][K] spectrograms):
  kernel_ms / gather_ms   specfilter_kernel and specfilter_gather_kernel from the library's per-launch event pairs;
  bytes_moved             what the call reads and writes — the waveform twice per window pair (8 x 2 per sample: every
                          sample lies in two windows), the gain rows once per window, the overlap-add rows written and
                          read once, y written — and a device copy_ of as many bytes beside it;
  materialised_ms         the same result for kind 'lsf' through two ilsf_device envelopes + kind 'spectrum', between two
                          events (in chunks of utterances at the large sizes): what the fused form saves, with the bytes of
                          the two envelopes that are never written;
  req_filter_kernel_ms    req_filter_kernel's time in a Requiem decode of the same frames: the yardstick for the shared
                          chain (window -> rfft -> minimum-phase response -> run sums).
Medians over --calls after --warmup.  Prints one JSON line.

    python tools/specfilter_bench.py [--calls 3] [--warmup 1] [--sizes 64x10@16000,1024x10@16000,16x60@48000]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-world_amd"))

P = 40


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


def made_lsf(rt, frames, seed):
    """[F][P + 1] = [log E, w_1 .. w_P]: ascending angles, evenly spread and moved by up to 0.35 of the spacing."""
    import torch

    g = torch.Generator(device=rt.device).manual_seed(seed)
    even = torch.arange(1, P + 1, device=rt.device, dtype=torch.float64) * (np.pi / (P + 1))
    w = even[None, :] + (torch.rand((frames, P), generator=g, device=rt.device, dtype=torch.float64) - 0.5) * (0.7 * np.pi / (P + 1))
    gain = torch.rand((frames, 1), generator=g, device=rt.device, dtype=torch.float64) * 4.0 - 8.0
    return torch.cat([gain, w], dim=1)


def size_case(wb, utts, seconds, fs, calls, warmup):
    import torch

    from world import lsf, specfilter
    from world.batch import BatchEncoding
    from world.compact import d4c_band_layout

    rt = wb.rt
    n = 1024 if fs <= 24000 else 2048
    k = n // 2 + 1
    hop = specfilter.default_hop(fs, 5)
    ny, nfu = int(seconds * fs), int(seconds * 200) + 1
    frames = utts * nfu
    x_off = np.arange(utts + 1, dtype=np.int64) * ny
    frame_off = np.arange(utts + 1, dtype=np.int64) * nfu
    g = torch.Generator(device=rt.device).manual_seed(7)
    x = torch.randn((utts * ny,), generator=g, device=rt.device, dtype=torch.float64)
    rows_n, rows_d = made_lsf(rt, frames, 1), made_lsf(rt, frames, 2)
    cos_n, cos_d = specfilter._lsf_cosine_rows(rt, rows_n), specfilter._lsf_cosine_rows(rt, rows_d)
    wmap = [specfilter.window_map(ny, nfu, hop, fs, 5)] * utts
    n_win = len(wmap[0])
    names = ("specfilter_kernel", "specfilter_gather_kernel")
    runf = 4 if n <= 1024 else 1
    row_doubles = utts * ((n_win + runf - 1) // runf) * ((runf - 1) * hop + n)

    def run(kind, num, den):
        return specfilter.filter_device(rt, x, x_off, fs, 5, n, num, den, kind=kind, frame_off=frame_off, hop=hop, window_map=wmap)

    def moved(cols):
        return 8 * (2 * utts * ny + 2 * utts * n_win * cols + 2 * row_doubles + utts * ny)

    def copy_ms(nbytes):
        src = torch.zeros((nbytes // 16,), device=rt.device, dtype=torch.float64)
        dst = torch.empty_like(src)
        ms = timed(lambda: dst.copy_(src), calls, warmup)
        del src, dst
        torch.cuda.empty_cache()
        return ms

    case = {"utterances": utts, "seconds": seconds, "fs": fs, "fft_size": n, "hop": hop, "windows": utts * n_win,
            "frames": frames, "row_bytes": 8 * row_doubles}
    ms = kernels_ms(rt, names, lambda: run("lsf", cos_n, cos_d), calls, warmup)
    y_lsf = run("lsf", cos_n, cos_d)
    b = moved(P + 1)
    cp = copy_ms(b)
    case["lsf"] = {"order": P, "kernel_ms": ms[names[0]], "gather_ms": ms[names[1]], "bytes_moved": b,
                   "gb_per_s": b / (ms[names[0]] + ms[names[1]]) / 1e6, "copy_same_bytes_ms": cp,
                   "over_copy": (ms[names[0]] + ms[names[1]]) / cp, "us_per_window": 1e3 * ms[names[0]] / (utts * n_win)}

    # the same through materialised envelopes, in chunks of utterances (two [chunk frames][K] envelopes at a time)
    chunk = max(1, min(utts, (1 << 28) // (nfu * k)))

    def materialised(keep=None):
        for u0 in range(0, utts, chunk):
            u1 = min(utts, u0 + chunk)
            f0, f1 = u0 * nfu, u1 * nfu
            sn, sd = lsf.ilsf_device(rt, rows_n[f0:f1], n), lsf.ilsf_device(rt, rows_d[f0:f1], n)
            y = specfilter.filter_device(rt, x[u0 * ny:u1 * ny], x_off[:u1 - u0 + 1], fs, 5, n, sn, sd, frame_off=frame_off[:u1 - u0 + 1],
                                         hop=hop, window_map=wmap[u0:u1])
            if keep is not None:
                keep[u0 * ny:u1 * ny] = y

    tm = timed(materialised, calls, warmup)
    want = torch.empty_like(y_lsf)
    materialised(want)
    case["lsf"]["materialised_ms"] = tm
    case["lsf"]["materialised_over_fused"] = tm / (ms[names[0]] + ms[names[1]])
    case["lsf"]["envelope_bytes_not_written"] = 2 * 8 * frames * k
    diff = (y_lsf - want).abs()
    case["lsf"]["max_abs_y"] = float(want.abs().max())
    case["lsf"]["max_abs_difference_to_materialised"] = float(diff.max())
    case["lsf"]["samples_that_differ"] = int((diff > 0).sum())
    case["lsf"]["relative_difference_to_materialised"] = float(diff.max() / want.abs().max())
    del diff
    del want, y_lsf
    torch.cuda.empty_cache()

    # kind 'spectrum' on one chunk's worth of resident spectrograms, scaled by nothing: the whole batch when it fits
    spec_utts = utts if 2 * 8 * frames * k <= (48 << 30) else chunk
    f1 = spec_utts * nfu
    sn, sd = lsf.ilsf_device(rt, rows_n[:f1], n), lsf.ilsf_device(rt, rows_d[:f1], n)

    def run_spec():
        return specfilter.filter_device(rt, x[:spec_utts * ny], x_off[:spec_utts + 1], fs, 5, n, sn, sd,
                                        frame_off=frame_off[:spec_utts + 1], hop=hop, window_map=wmap[:spec_utts])

    ms = kernels_ms(rt, names, run_spec, calls, warmup)
    b = 8 * (2 * spec_utts * ny + 2 * spec_utts * n_win * k + 2 * (row_doubles // utts) * spec_utts + spec_utts * ny)
    cp = copy_ms(b)
    case["spectrum"] = {"utterances": spec_utts, "kernel_ms": ms[names[0]], "gather_ms": ms[names[1]], "bytes_moved": b,
                        "gb_per_s": b / (ms[names[0]] + ms[names[1]]) / 1e6, "copy_same_bytes_ms": cp,
                        "over_copy": (ms[names[0]] + ms[names[1]]) / cp,
                        "us_per_window": 1e3 * ms[names[0]] / (spec_utts * n_win)}

    # the yardstick: req_filter_kernel in a Requiem decode of the same frames (spectrogram sn, every frame voiced at 120 Hz)
    _, nap = d4c_band_layout(fs, True)
    batch = rt.make_batch(np.zeros(spec_utts + 1, dtype=np.int64), frame_off[:spec_utts + 1])
    tp = torch.arange(nfu, dtype=torch.float64, device=rt.device).mul_(0.005).repeat(spec_utts)
    ones = torch.ones((f1,), dtype=torch.float64, device=rt.device)
    enc = BatchEncoding(rt, batch, fs, tp, ones * 120.0, ones.clone(), sn,
                        torch.full((f1, nap + 2), -20.0, dtype=torch.float64, device=rt.device), n, True, 5)
    rq = kernels_ms(rt, ("req_filter_kernel", "req_gather_kernel"), lambda: wb.decode_device(enc, check=False), calls, warmup)
    wb.check()
    case["requiem_yardstick"] = {"utterances": spec_utts, "req_filter_kernel_ms": rq["req_filter_kernel"],
                                 "req_gather_kernel_ms": rq["req_gather_kernel"],
                                 "us_per_frame": 1e3 * rq["req_filter_kernel"] / max(1, spec_utts * (nfu - 3)),
                                 "specfilter_spectrum_over_req_filter_per_window":
                                     case["spectrum"]["us_per_window"] / (1e3 * rq["req_filter_kernel"] / max(1, spec_utts * (nfu - 3)))}
    del enc, sn, sd, x
    torch.cuda.empty_cache()
    rt.trim()
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="64x10@16000,1024x10@16000,16x60@48000")
    a = ap.parse_args()
    from world.batch import WorldBatch

    wb = WorldBatch(0, prefetch_timebase=False)
    out = {"calls": a.calls, "warmup": a.warmup, "sizes": {}}
    for s in a.sizes.split(","):
        shape, fs = s.split("@")
        utts, seconds = shape.split("x")
        out["sizes"][s] = size_case(wb, int(utts), float(seconds), int(fs), a.calls, a.warmup)
    assert wb.rt.take_flags() == [0] * 16
    print(json.dumps(out))


if __name__ == "__main__":
    main()
