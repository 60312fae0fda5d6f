"""Batched MLPG (world/dynamics.py) at the corpus sizes: 64 and 1024 utterances of 10 s (2001 frames of the 5 ms
grid), three windows of half-width 1 (static, delta, delta-delta), at d = 40 (a mel-cepstrum) and d = 1 (log-f0), on
resident random means and per-frame variances (no model: the kernel does not care where they came from).  Per case: the
kernel time of wh_mlpg and of wh_delta_features from the library's per-launch event pairs, the bytes the MLPG kernel
moves — means and variances read, multipliers written and read back, the output written, read back and written again —
and, in the same run, the time of a device copy_ that moves as many bytes (half of them read, half written), so that
time / copy time says how far the kernel is from the memory system's rate; systems per second; and for context
scipy.linalg.solveh_banded per system on one host core (the matrix already assembled).  Medians over --calls after
--warmup.  Prints one JSON line.

    python tools/mlpg_bench.py [--calls 5] [--warmup 1] [--utts 64,1024] [--frames 2001] [--ds 40,1]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-world_amd"))


def med(v):
    return float(np.median(v))


def case(rt, utts, frames, d, calls, warmup):
    import torch

    from world.dynamics import HTS_WINDOWS, delta_features_device, mlpg_device, plan_groups, workspace_bytes

    n_win, half = 3, 1
    F = utts * frames
    off = np.arange(utts + 1, dtype=np.int64) * frames
    batch = rt.make_batch(np.zeros(utts + 1, dtype=np.int64), off)
    g = torch.Generator(device=rt.device).manual_seed(1)
    x = torch.randn((F, d), generator=g, device=rt.device, dtype=torch.float64).cumsum(0)
    var = torch.exp(torch.randn((F, n_win * d), generator=g, device=rt.device, dtype=torch.float64))
    kern = {"mlpg_kernel": [], "delta_features_kernel": []}
    err = None
    for i in range(warmup + calls):
        if i == warmup:
            torch.cuda.synchronize()
            rt.profile(True)
        mean = delta_features_device(rt, batch, x, HTS_WINDOWS)
        c = mlpg_device(rt, batch, mean, var, HTS_WINDOWS)
        if i >= warmup:
            rec = rt.profile_collect()
            for name in kern:
                kern[name].append(sum(ms for nm, ms in rec if nm.startswith(name)))
        err = float((c - x).abs().max().cpu())
    rt.profile(False)
    B = 2 * half
    moved = 8 * F * d * (2 * n_win + 2 * B + 3)
    src = torch.empty((moved // 16,), device=rt.device, dtype=torch.float64).normal_(generator=g)
    dst = torch.empty_like(src)
    copies = []
    for i in range(warmup + calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        e1.synchronize()
        if i >= warmup:
            copies.append(e0.elapsed_time(e1))
    ms = med(kern["mlpg_kernel"])
    res = {"utterances": utts, "frames": frames, "d": d, "n_win": n_win, "half": half, "systems": utts * d,
           "waves": (utts * d + 63) // 64, "groups": len(plan_groups([frames] * utts, d, half)),
           "workspace_bytes": workspace_bytes(F, d, half), "mlpg_kernel_ms": ms,
           "delta_features_kernel_ms": med(kern["delta_features_kernel"]), "bytes_moved": moved,
           "copy_same_bytes_ms": med(copies), "mlpg_over_copy": ms / med(copies),
           "mlpg_gbytes_per_s": moved / ms / 1e6, "copy_gbytes_per_s": moved / med(copies) / 1e6,
           "systems_per_s": utts * d / ms * 1e3, "ns_per_step_per_wave": ms * 1e6 / frames,
           "max_abs_track_error_unit_model": err}
    del x, var, mean, c, src, dst
    torch.cuda.empty_cache()
    return res


def host_solveh_banded(frames, n=200):
    """Seconds per system of scipy.linalg.solveh_banded on one core: a 2001 x 2001 matrix of half-bandwidth 2."""
    from scipy.linalg import solveh_banded

    rng = np.random.RandomState(0)
    ab = np.zeros((3, frames))
    ab[0] = 6.0 + rng.rand(frames)
    ab[1, :-1] = rng.rand(frames - 1) - 0.5
    ab[2, :-2] = rng.rand(frames - 2) - 0.5
    r = rng.randn(frames)
    solveh_banded(ab, r, lower=True)
    t0 = time.perf_counter()
    for _ in range(n):
        solveh_banded(ab, r, lower=True)
    return (time.perf_counter() - t0) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--utts", default="64,1024")
    ap.add_argument("--frames", type=int, default=2001)
    ap.add_argument("--ds", default="40,1")
    a = ap.parse_args()
    from world import _hip

    rt = _hip.Runtime.get(0)
    out = {"frames": a.frames, "calls": a.calls, "cases": {}}
    for utts in (int(v) for v in a.utts.split(",")):
        for d in (int(v) for v in a.ds.split(",")):
            out["cases"]["%dx%dx%d" % (utts, a.frames, d)] = case(rt, utts, a.frames, d, a.calls, a.warmup)
    assert rt.take_flags() == [0] * 16
    sec = host_solveh_banded(a.frames)
    out["host_solveh_banded_us_per_system"] = sec * 1e6
    for c in out["cases"].values():
        c["host_one_core_s_for_the_batch"] = sec * c["systems"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
