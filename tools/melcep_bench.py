"""wh_melcep_filter (world/melcep.py) at corpus sizes, on resident made tensors: 64 and 1024 utterances of
10 s at 16 kHz (N = 1024, hop 80, orders 24 and 40, alpha 0.42) and 16 of 60 s at 48 kHz (N = 2048, hop 240, order 59,
alpha 0.554), rows on the 5 ms grid.

Per size and order, all in this one run:
  closed            wh_melcep_filter: specfilter_kernel and specfilter_gather_kernel from the library's per-launch event
                    pairs, the bytes the call moves and a device copy_ of as many bytes beside it;
  materialised_ms   the same result through two spectrum_device envelopes + wh_spectral_filter kind 0, between two events
                    (in chunks of utterances at the large sizes), with the bytes of the two envelopes that the closed form
                    never writes and the difference of the two results;
  kind0_alone       wh_spectral_filter kind 0 on resident envelopes (one chunk's worth), per window;
  kind1             wh_spectral_filter kind 1 at p = 40 on made rows, per window.
And once, at 2 049 024 frames of 513 bins: the coding and the decoding product (melcep_device, spectrum_device), orders 24
and 40, against a device copy_ of the bytes each reads and writes.
Medians over --calls after --warmup.  Prints one JSON line.

    python tools/melcep_bench.py [--calls 5] [--warmup 1] [--sizes 64x10@16000,1024x10@16000,16x60@48000] [--no-products]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-world_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from specfilter_bench import kernels_ms, made_lsf, timed  # noqa: E402  (the same timers as the record it is read beside)

NAMES = ("specfilter_kernel", "specfilter_gather_kernel")
ORDERS = {16000: (24, 40), 48000: (59,)}
PRODUCT_FRAMES = 2049024


def made_rows(rt, frames, m, seed):
    """c[0] ~ 2 N(0, 1), c[j] ~ N(0, 1) / j."""
    import torch

    g = torch.Generator(device=rt.device).manual_seed(seed)
    c = torch.randn((frames, m + 1), generator=g, device=rt.device, dtype=torch.float64)
    c[:, 0] *= 2.0
    c[:, 1:] /= torch.arange(1, m + 1, device=rt.device, dtype=torch.float64)[None, :]
    return c


def copy_ms(rt, nbytes, calls, warmup):
    import torch

    src = torch.zeros((nbytes // 16,), device=rt.device, dtype=torch.float64)
    dst = torch.empty_like(src)
    ms = timed(lambda: dst.copy_(src), calls, warmup)
    del src, dst
    torch.cuda.empty_cache()
    return ms


def size_case(wb, utts, seconds, fs, calls, warmup):
    import torch

    from world import melcep, specfilter

    rt = wb.rt
    n = 1024 if fs <= 24000 else 2048
    k = n // 2 + 1
    alpha = melcep.default_alpha(fs)
    hop = specfilter.default_hop(fs, 5)
    ny, nfu = int(seconds * fs), int(seconds * 200) + 1
    frames = utts * nfu
    x_off = np.arange(utts + 1, dtype=np.int64) * ny
    frame_off = np.arange(utts + 1, dtype=np.int64) * nfu
    g = torch.Generator(device=rt.device).manual_seed(7)
    x = torch.randn((utts * ny,), generator=g, device=rt.device, dtype=torch.float64)
    wmap = [specfilter.window_map(ny, nfu, hop, fs, 5)] * utts
    n_win = len(wmap[0])
    runf = 4 if n <= 1024 else 1
    row_doubles = utts * ((n_win + runf - 1) // runf) * ((runf - 1) * hop + n)
    chunk = max(1, min(utts, (1 << 28) // (nfu * k)))  # utterances whose two envelopes are resident at a time

    def moved(cols, u=utts):
        return 8 * (2 * u * ny + 2 * u * n_win * cols + 2 * (row_doubles // utts) * u + u * ny)

    def geometry(u0, u1):
        return dict(frame_off=frame_off[:u1 - u0 + 1], hop=hop, window_map=wmap[u0:u1])

    case = {"utterances": utts, "seconds": seconds, "fs": fs, "fft_size": n, "hop": hop, "alpha": alpha, "windows": utts * n_win,
            "frames": frames, "row_bytes": 8 * row_doubles, "chunk_utterances": chunk, "orders": {}}
    for m in ORDERS[48000 if fs > 24000 else 16000]:
        num, den = made_rows(rt, frames, m, 1), made_rows(rt, frames, m, 2)

        def closed():
            return melcep.filter_device(rt, x, x_off, fs, 5, n, num, den, alpha, **geometry(0, utts))

        ms = kernels_ms(rt, NAMES, closed, calls, warmup)
        y_closed = closed()
        b = moved(m + 1)
        cp = copy_ms(rt, b, calls, warmup)
        tot = ms[NAMES[0]] + ms[NAMES[1]]
        rec = {"kernel_ms": ms[NAMES[0]], "gather_ms": ms[NAMES[1]], "bytes_moved": b, "gb_per_s": b / tot / 1e6,
               "copy_same_bytes_ms": cp, "over_copy": tot / cp, "us_per_window": 1e3 * ms[NAMES[0]] / (utts * n_win)}

        def materialised(keep=None):
            for u0 in range(0, utts, chunk):
                u1 = min(utts, u0 + chunk)
                f0, f1 = u0 * nfu, u1 * nfu
                sn, sd = melcep.spectrum_device(rt, num[f0:f1], n, alpha), melcep.spectrum_device(rt, den[f0:f1], n, alpha)
                y = specfilter.filter_device(rt, x[u0 * ny:u1 * ny], x_off[:u1 - u0 + 1], fs, 5, n, sn, sd, **geometry(u0, u1))
                if keep is not None:
                    keep[u0 * ny:u1 * ny] = y

        tm = timed(materialised, calls, warmup)
        want = torch.empty_like(y_closed)
        materialised(want)
        diff = (y_closed - want).abs()
        rec.update({"materialised_ms": tm, "materialised_over_closed": tm / tot, "envelope_bytes_not_written": 2 * 8 * frames * k,
                    "relative_difference_to_materialised": float(diff.max() / want.abs().max())})
        del diff, want, y_closed
        torch.cuda.empty_cache()

        # kind 0 alone, on one chunk's worth of resident envelopes
        f1 = chunk * nfu
        sn, sd = melcep.spectrum_device(rt, num[:f1], n, alpha), melcep.spectrum_device(rt, den[:f1], n, alpha)
        ms0 = kernels_ms(rt, NAMES, lambda: specfilter.filter_device(rt, x[:chunk * ny], x_off[:chunk + 1], fs, 5, n, sn, sd,
                                                                     **geometry(0, chunk)), calls, warmup)
        rec["kind0_alone"] = {"utterances": chunk, "kernel_ms": ms0[NAMES[0]], "gather_ms": ms0[NAMES[1]],
                              "us_per_window": 1e3 * ms0[NAMES[0]] / (chunk * n_win)}
        rec["closed_over_kind0_alone_per_window"] = rec["us_per_window"] / rec["kind0_alone"]["us_per_window"]
        del sn, sd, num, den
        torch.cuda.empty_cache()
        case["orders"][str(m)] = rec

    # kind 1 at p = 40 (the rows' cosines), the whole batch
    cos_n, cos_d = (specfilter._lsf_cosine_rows(rt, made_lsf(rt, frames, s)) for s in (1, 2))
    ms1 = kernels_ms(rt, NAMES, lambda: specfilter.filter_device(rt, x, x_off, fs, 5, n, cos_n, cos_d, kind="lsf", **geometry(0, utts)),
                     calls, warmup)
    case["kind1_p40"] = {"kernel_ms": ms1[NAMES[0]], "gather_ms": ms1[NAMES[1]], "us_per_window": 1e3 * ms1[NAMES[0]] / (utts * n_win)}
    del cos_n, cos_d, x
    torch.cuda.empty_cache()
    rt.trim()
    return case


def products(wb, calls, warmup):
    """melcep_device and spectrum_device at PRODUCT_FRAMES frames of 513 bins."""
    import torch

    from world import melcep

    rt = wb.rt
    k, f = 513, PRODUCT_FRAMES
    g = torch.Generator(device=rt.device).manual_seed(3)
    spec = torch.rand((f, k), generator=g, device=rt.device, dtype=torch.float64).mul_(6.0).sub_(3.0).exp_()
    out = {"frames": f, "k_bins": k, "alpha": 0.42, "orders": {}}
    for m in (24, 40):
        rows = made_rows(rt, f, m, 4)
        b = 8 * f * (k + m + 1)
        enc = timed(lambda: melcep.melcep_device(rt, spec, m, 0.42), calls, warmup)
        dec = timed(lambda: melcep.spectrum_device(rt, rows, 1024, 0.42), calls, warmup)
        cp = copy_ms(rt, b, calls, warmup)
        out["orders"][str(m)] = {"bytes": b, "encode_ms": enc, "decode_ms": dec, "copy_same_bytes_ms": cp,
                                 "encode_over_copy": enc / cp, "decode_over_copy": dec / cp}
        del rows
        torch.cuda.empty_cache()
    del spec
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="64x10@16000,1024x10@16000,16x60@48000")
    ap.add_argument("--no-products", action="store_true")
    a = ap.parse_args()
    from world.batch import WorldBatch

    wb = WorldBatch(0, prefetch_timebase=False)
    out = {"calls": a.calls, "warmup": a.warmup, "sizes": {}}
    for s in a.sizes.split(","):
        shape, fs = s.split("@")
        utts, seconds = shape.split("x")
        out["sizes"][s] = size_case(wb, int(utts), float(seconds), int(fs), a.calls, a.warmup)
    if not a.no_products:
        out["products"] = products(wb, a.calls, a.warmup)
    assert wb.rt.take_flags() == [0] * 16
    print(json.dumps(out))


if __name__ == "__main__":
    main()
