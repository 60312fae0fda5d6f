"""Line spectral frequencies (world/lsf.py) at the corpus sizes: 128 064 and 2 049 024 frames (64 and 1024
utterances of 10 s on the 5 ms grid) of K = 513 bins, at orders 24, 40 and 64, on resident made spectra (five formant-like
peaks per frame over a floor, 60 dB of range).  Per case the time of each of the four kernels from the library's
per-launch event pairs — the autocorrelation product (feature_matmul_kernel), lpc_levinson_kernel, lsf_from_lpc_kernel,
lsf_envelope_kernel — the bytes each moves (rows read plus rows written), and, in the same run, the time of a device
copy_ that moves as many bytes (half read, half written): time / copy time says how far a kernel is from the memory
system's rate.  For context the NumPy reference (tests/_lsf_reference.py, the same arithmetic) per frame on one host core,
and the distribution of grid levels.  Medians over --calls after --warmup.  Prints one JSON line.

    python tools/lsf_bench.py [--calls 5] [--warmup 1] [--frames 128064,2049024] [--orders 24,40,64] [--bins 513]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-world_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

KERNELS = ("feature_matmul_kernel", "lpc_levinson_kernel", "lsf_from_lpc_kernel", "lsf_envelope_kernel")


def med(v):
    return float(np.median(v))


def made_spectra(rt, frames, k_bins, seed=1):
    import torch

    g = torch.Generator(device=rt.device).manual_seed(seed)
    rnd = lambda lo, hi: torch.rand((frames, 1), generator=g, device=rt.device, dtype=torch.float64) * (hi - lo) + lo  # noqa: E731
    w = torch.linspace(0, np.pi, k_bins, device=rt.device, dtype=torch.float64)[None, :]
    s = torch.full((frames, k_bins), 1e-3, device=rt.device, dtype=torch.float64)
    for _ in range(5):
        t = (w - rnd(0.1, 3.0)) / rnd(0.02, 0.3)
        t.mul_(t).add_(1.0).reciprocal_().mul_(rnd(0.1, 10.0))
        s.add_(t)
        del t
    return s


def copy_ms(rt, n_bytes, calls, warmup):
    import torch

    src = torch.zeros((max(n_bytes // 16, 1),), device=rt.device, dtype=torch.float64)
    dst = torch.empty_like(src)
    out = []
    for i in range(warmup + calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        e1.synchronize()
        if i >= warmup:
            out.append(e0.elapsed_time(e1))
    return med(out)


def case(rt, spec, p, calls, warmup):
    import torch

    from world import lsf

    frames, k_bins = (int(v) for v in spec.shape)
    kern = {name: [] for name in KERNELS}
    level = None
    for i in range(warmup + calls):
        if i == warmup:
            torch.cuda.synchronize()
            rt.profile(True)
        r = lsf.autocorr_device(rt, spec, p)
        a, e, _ = lsf.levinson_device(rt, r, p)
        x, level = lsf.lsf_from_lpc_device(rt, a, want_level=True)
        env = lsf.envelope_device(rt, torch.cat([e[:, None], x], dim=1), k_bins)
        if i >= warmup:
            rec = rt.profile_collect()
            for name in kern:
                kern[name].append(sum(ms for nm, ms in rec if nm.startswith(name)))
        del env
    rt.profile(False)
    levels = {int(k): int(v) for k, v in zip(*np.unique(level.cpu().numpy(), return_counts=True))}
    row = 8 * frames
    moved = {"feature_matmul_kernel": row * (k_bins + p + 1), "lpc_levinson_kernel": row * (2 * (p + 1) + 1),
             "lsf_from_lpc_kernel": row * (2 * p + 1), "lsf_envelope_kernel": row * (p + 1 + k_bins)}
    res = {"frames": frames, "k_bins": k_bins, "order": p, "grid_levels": levels, "kernels": {}}
    for name in KERNELS:
        ms, cp = med(kern[name]), copy_ms(rt, moved[name], calls, warmup)
        res["kernels"][name] = {"ms": ms, "bytes_moved": moved[name], "copy_same_bytes_ms": cp, "over_copy": ms / cp,
                                "ns_per_frame": ms * 1e6 / frames}
    res["chain_ms"] = sum(v["ms"] for v in res["kernels"].values())
    torch.cuda.empty_cache()
    return res


def host_reference(spec_h, p):
    """Seconds per frame of the NumPy reference on one core: (encode = lags, recursion, roots; decode = envelope)."""
    import _lsf_reference as ref

    k_bins = spec_h.shape[1]
    t0 = time.perf_counter()
    rows, _, _ = ref.lsf_rows(ref.autocorr(spec_h, p), p)
    t1 = time.perf_counter()
    ref.ilsf_rows(rows, k_bins)
    t2 = time.perf_counter()
    return (t1 - t0) / len(spec_h), (t2 - t1) / len(spec_h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", default="128064,2049024")
    ap.add_argument("--orders", default="24,40,64")
    ap.add_argument("--bins", type=int, default=513)
    ap.add_argument("--host-frames", type=int, default=512)
    a = ap.parse_args()
    from world import _hip

    rt = _hip.Runtime.get(0)
    orders = [int(v) for v in a.orders.split(",")]
    out = {"calls": a.calls, "cases": {}, "host_numpy_us_per_frame": {}}
    for frames in (int(v) for v in a.frames.split(",")):
        spec = made_spectra(rt, frames, a.bins)
        for p in orders:
            out["cases"]["%dx%d p=%d" % (frames, a.bins, p)] = case(rt, spec, p, a.calls, a.warmup)
        host = spec[:a.host_frames].cpu().numpy()
        del spec
    assert rt.take_flags() == [0] * 16
    for p in orders:
        enc, dec = host_reference(host, p)
        out["host_numpy_us_per_frame"]["p=%d" % p] = {"encode": enc * 1e6, "decode": dec * 1e6}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
