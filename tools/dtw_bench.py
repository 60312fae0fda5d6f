"""Batched DTW (world/align.py) at the corpus sizes: 64 and 1024 pairs of 10 s x 10 s (2001 x 2001 frames,
d = 39: mel-cepstral coefficients 1..39 of the 5 ms grid) of resident random rows (no encode: the kernel does not care
where its rows came from), the whole rectangle and radius = 200.  Per case: kernel time of wh_dtw from the library's
per-launch event pairs (dtw_recurrence_kernel, dtw_backtrack_kernel, dtw_reverse_kernel), cells per second over the
recurrence kernel — cells of the rectangle, and under the band the cells inside it — and the share of the FP64 issue
rate those cells stand for: 3 d FP64 instructions per cell (a subtraction, a product and a sum per column) against the
vector ceiling bench.py counts with (FP64_VECTOR_PEAK_TFLOPS / 2 flop per FMA: 256 CUs x 4 SIMDs x 16 lanes per clock at
2.4 GHz).  Medians over --calls after --warmup.  Prints one JSON line.

    python tools/dtw_bench.py [--calls 5] [--warmup 1] [--pairs 64,1024] [--frames 2001] [--d 39]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-world_amd"))

FP64_ISSUE_PEAK = 78.6e12 / 2  # FP64 vector instructions x lanes per second (bench.py: FP64_VECTOR_PEAK_TFLOPS)
KERNELS = ("dtw_recurrence_kernel", "dtw_backtrack_kernel", "dtw_reverse_kernel")


def med(v):
    return float(np.median(v))


def cells_in_band(n, m, radius):
    if radius is None:
        return n * m
    i = np.arange(n, dtype=np.int64)[:, None]
    j = np.arange(m, dtype=np.int64)[None, :]
    return int(np.sum(np.abs(j * (n - 1) - i * (m - 1)) <= radius * max(n - 1, m - 1)))


def case(rt, pairs, frames, d, radius, calls, warmup):
    import torch

    from world.align import align_device, pair_workspace_bytes, plan_groups

    off = np.arange(pairs + 1, dtype=np.int64) * frames
    ba = rt.make_batch(np.zeros(pairs + 1, dtype=np.int64), off)
    bb = rt.make_batch(np.zeros(pairs + 1, dtype=np.int64), off)
    g = torch.Generator(device=rt.device).manual_seed(1)
    xa = torch.randn((pairs * frames, d), generator=g, device=rt.device, dtype=torch.float64)
    xb = torch.randn((pairs * frames, d), generator=g, device=rt.device, dtype=torch.float64)
    kern = {name: [] for name in KERNELS}
    mean_cost = None
    for i in range(warmup + calls):
        if i == warmup:
            torch.cuda.synchronize()
            rt.profile(True)
        al = align_device(rt, ba, xa, bb, xb, radius=radius)
        if i >= warmup:
            rec = rt.profile_collect()
            for name in kern:
                kern[name].append(sum(ms for nm, ms in rec if nm.startswith(name)))
        mean_cost = float(al.mean_cost().mean().cpu())
    rt.profile(False)
    rec_ms = med(kern["dtw_recurrence_kernel"])
    inside = cells_in_band(frames, frames, radius)
    res = {"pairs": pairs, "frames": frames, "d": d, "radius": radius,
           "groups": len(plan_groups([frames] * pairs, [frames] * pairs)),
           "workspace_bytes": pairs * pair_workspace_bytes(frames, frames),
           "recurrence_kernel_ms": rec_ms, "backtrack_kernel_ms": med(kern["dtw_backtrack_kernel"]),
           "reverse_kernel_ms": med(kern["dtw_reverse_kernel"]), "kernel_ms": sum(med(v) for v in kern.values()),
           "cells_rectangle": pairs * frames * frames, "cells_in_band": pairs * inside, "mean_cost": mean_cost}
    res["rectangle_cells_per_s"] = res["cells_rectangle"] / rec_ms * 1e3
    res["band_cells_per_s"] = res["cells_in_band"] / rec_ms * 1e3
    res["fp64_issue_frac"] = res["band_cells_per_s"] * 3 * d * 1.0 / FP64_ISSUE_PEAK
    res["pairs_per_s"] = pairs / res["kernel_ms"] * 1e3
    del xa, xb, al
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pairs", default="64,1024")
    ap.add_argument("--frames", type=int, default=2001)
    ap.add_argument("--d", type=int, default=39)
    ap.add_argument("--radius", type=int, default=200)
    a = ap.parse_args()
    from world import _hip

    rt = _hip.Runtime.get(0)
    out = {"frames": a.frames, "d": a.d, "calls": a.calls, "fp64_issue_peak_per_s": FP64_ISSUE_PEAK, "cases": {}}
    for pairs in (int(v) for v in a.pairs.split(",")):
        for radius in (None, a.radius):
            name = "%dx%dx%d_%s" % (pairs, a.frames, a.frames, "full" if radius is None else "radius%d" % radius)
            out["cases"][name] = case(rt, pairs, a.frames, a.d, radius, a.calls, a.warmup)
    assert rt.take_flags() == [0] * 16
    print(json.dumps(out))


if __name__ == "__main__":
    main()
