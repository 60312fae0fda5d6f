"""The two per-frame steps of a chain over line spectral frequencies (world/lsf.py) at the corpus size:
2 049 024 frames (1024 utterances of 10 s on the 5 ms grid), on resident made rows.

repair      wh_lsf_repair on [F][p + 1] rows (the angles are columns 1 .. p), p = 24 / 40 / 64, every row in need of the
            repair (angles in random order).  Kernel time from the library's per-launch event pairs; beside it, in the
            same run, a device copy_ of the bytes it moves (F p doubles read, F p written) and world.lsf.repair_rows —
            the torch statement the kernel replaced, about 2 p + 2 launches — on the same tensor, between two events.
distortion  wh_lsf_distortion on F pairs of rows, p = 40, K = 513 and K = 1025, against what it replaces: envelope_device
            on both sides followed by torch's log / mean, in chunks of --chunk frames (two [chunk][K] envelopes at a
            time), between two events.  The kernel's FP64 work per pair and bin is 2 p subtractions + 2 p multiplies for
            the four products and 17 further operations, the logarithm apart: flops / time is set against the FP64
            vector rate (256 CUs x 128 flop / clock as FMA, 2.4 GHz: 78.6 Tflop/s; a kernel without FMA — this one is
            built with -ffp-contract=off — has half of that to use).

Medians over --calls after --warmup.  Prints one JSON line.

    python tools/lsf_chain_bench.py [--calls 5] [--warmup 1] [--frames 2049024] [--orders 24,40,64] [--bins 513,1025]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-world_amd"))

FP64_VECTOR_TFLOPS = 256 * 128 * 2.4e9 / 1e12


def med(v):
    return float(np.median(v))


def timed(fn, calls, warmup):
    """Median milliseconds of fn() between two events on the current stream."""
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


def kernel_ms(rt, name, fn, calls, warmup):
    """Median milliseconds of the kernel ``name`` over calls of fn(), from the library's event pairs."""
    import torch

    out = []
    for i in range(warmup + calls):
        if i == warmup:
            torch.cuda.synchronize()
            rt.profile(True)
        fn()
        if i >= warmup:
            out.append(sum(ms for nm, ms in rt.profile_collect() if nm.startswith(name)))
    rt.profile(False)
    return med(out)


def made_rows(rt, frames, p, seed, ordered):
    """[F][p + 1]: a gain and p angles inside (0, pi) — ascending, or as drawn."""
    import torch

    g = torch.Generator(device=rt.device).manual_seed(seed)
    w = torch.rand((frames, p), generator=g, device=rt.device, dtype=torch.float64) * (np.pi - 0.04) + 0.02
    if ordered:
        w = torch.sort(w, dim=1).values
    gain = torch.rand((frames, 1), generator=g, device=rt.device, dtype=torch.float64) * 10.0 - 8.0
    return torch.cat([gain, w], dim=1)


def repair_case(rt, frames, p, calls, warmup):
    import torch

    from world import lsf

    rows = made_rows(rt, frames, p, p, ordered=False)
    gap = 0.3 / (p + 2)
    out = torch.empty((frames, p), device=rt.device, dtype=torch.float64)
    ms = kernel_ms(rt, "lsf_repair_kernel", lambda: lsf.repair_device(rt, rows[:, 1:], gap, out=out), calls, warmup)
    want = lsf.repair_rows(torch, rows[:, 1:], gap)
    same = bool(torch.equal(out, want))
    del want
    src = torch.zeros((frames * p,), device=rt.device, dtype=torch.float64)
    dst = torch.empty_like(src)
    cp = timed(lambda: dst.copy_(src), calls, warmup)
    del src, dst
    tm = timed(lambda: lsf.repair_rows(torch, rows[:, 1:], gap), calls, warmup)
    torch.cuda.empty_cache()
    moved = 16 * frames * p
    return {"frames": frames, "order": p, "kernel_ms": ms, "bytes_moved": moved, "gb_per_s": moved / ms / 1e6,
            "copy_same_bytes_ms": cp, "over_copy": ms / cp, "torch_repair_rows_ms": tm, "torch_over_kernel": tm / ms,
            "same_bits_as_repair_rows": same}


def distortion_case(rt, frames, p, k_bins, chunk, calls, warmup):
    import torch

    from world import lsf

    a = made_rows(rt, frames, p, 100 + p, ordered=True)
    b = made_rows(rt, frames, p, 200 + p, ordered=True)
    ex_a = torch.cat([torch.exp(a[:, :1]), torch.cos(a[:, 1:])], dim=1)  # [E, x ..], as envelope_device takes them
    ex_b = torch.cat([torch.exp(b[:, :1]), torch.cos(b[:, 1:])], dim=1)
    ms = kernel_ms(rt, "lsf_distortion_kernel", lambda: lsf.distortion_sums_device(rt, ex_a, ex_b, k_bins), calls, warmup)
    got = lsf.distortion_db(torch, a[:, 0] - b[:, 0], *lsf.distortion_sums_device(rt, ex_a, ex_b, k_bins).unbind(1), k_bins,
                            gain=False)

    def materialised():
        out = torch.empty((frames,), device=rt.device, dtype=torch.float64)
        for f0 in range(0, frames, chunk):
            f1 = min(frames, f0 + chunk)
            d = torch.log(lsf.envelope_device(rt, ex_a[f0:f1], k_bins) / lsf.envelope_device(rt, ex_b[f0:f1], k_bins))
            d -= d.mean(dim=1, keepdim=True)  # (gain-free, as Alignment.lsd_db scores)
            out[f0:f1] = lsf.LSD_SCALE * torch.sqrt((d * d).mean(dim=1))
        return out

    tm = timed(materialised, calls, warmup)
    want = materialised()
    # (E cancels in the gain-free score only up to the envelope's own division: compare loosely, it is a bench)
    worst = float((got - want).abs().max() / want.abs().max())
    del want
    torch.cuda.empty_cache()
    flops = frames * k_bins * (4 * p + 17)
    return {"pairs": frames, "order": p, "k_bins": k_bins, "kernel_ms": ms, "fp64_flops_without_log": flops,
            "tflops": flops / ms / 1e9, "share_of_fp64_vector_fma_rate": flops / ms / 1e9 / FP64_VECTOR_TFLOPS,
            "share_of_fp64_vector_issue_rate": flops / ms / 1e9 / (FP64_VECTOR_TFLOPS / 2),
            "envelopes_log_mean_ms": tm, "chunk": chunk, "materialised_over_kernel": tm / ms,
            "envelope_bytes_not_written": 2 * 8 * frames * k_bins, "relative_difference_to_materialised": worst}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=2049024)
    ap.add_argument("--orders", default="24,40,64")
    ap.add_argument("--bins", default="513,1025")
    ap.add_argument("--dist-order", type=int, default=40)
    ap.add_argument("--chunk", type=int, default=131072)
    a = ap.parse_args()
    from world import _hip

    rt = _hip.Runtime.get(0)
    out = {"calls": a.calls, "warmup": a.warmup, "repair": {}, "distortion": {}}
    for p in (int(v) for v in a.orders.split(",")):
        out["repair"]["%d p=%d" % (a.frames, p)] = repair_case(rt, a.frames, p, a.calls, a.warmup)
    for k in (int(v) for v in a.bins.split(",")):
        out["distortion"]["%d p=%d K=%d" % (a.frames, a.dist_order, k)] = distortion_case(rt, a.frames, a.dist_order, k,
                                                                                         a.chunk, a.calls, a.warmup)
    assert rt.take_flags() == [0] * 16
    print(json.dumps(out))


if __name__ == "__main__":
    main()
