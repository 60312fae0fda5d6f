"""Device time of wh_resample_poly at the corpus sizes: 1024 x 10 s of resident float64 from 44.1 and from
48 kHz to 16 kHz, and 16 -> 48 kHz on 1024 x 10 s of output.  Per case: the median over >= 20 calls (after warm-up) of
the kernel time (the library's per-launch event pairs) and of the whole call between two stream events; bytes and
multiplies + adds counted from the shapes, the rate as a fraction of the HBM floor (6.29 TB/s copy rate) and of the
FP64 issue floor (one wave-wide multiply or add per clock per CU, 256 CUs at 2.4 GHz); scipy on the host timed on one
utterance in the same run.  Prints one JSON line.

    python tools/resample_bench.py [--calls 20] [--warmup 3] [--utts 1024]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-world_amd"))

HBM_BPS = 6.29e12
FP64_OPS = 256 * 2.4e9 * 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--utts", type=int, default=1024)
    a = ap.parse_args()
    import torch
    from scipy import signal

    from world import _hip
    from world.resample import design, rates_ratio, resample_device

    rt = _hip.Runtime.get()
    out = {"utts": a.utts, "calls": a.calls, "cases": {}}
    for name, fs_in, fs_out, n_in in (("44k1_to_16k", 44100, 16000, 441000), ("48k_to_16k", 48000, 16000, 480000),
                                      ("16k_to_48k", 16000, 48000, 160000)):
        up, down = rates_ratio(fs_in, fs_out)
        d = design(up, down, n_in)
        x_d = torch.randn(a.utts * n_in, dtype=torch.float64, device=rt.device)
        off = np.arange(a.utts + 1, dtype=np.int64) * n_in
        y_d = None
        for _ in range(a.warmup):
            y_d, yo = resample_device(rt, x_d, off, up, down)
        torch.cuda.synchronize()
        call_ms, kern_ms = [], []
        rt.profile(True)
        for _ in range(a.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            y_d, yo = resample_device(rt, x_d, off, up, down)
            e1.record()
            e1.synchronize()
            call_ms.append(e0.elapsed_time(e1))
            kern_ms.append(sum(ms for nm, ms in rt.profile_collect() if nm.startswith("resample_kernel")))
        rt.profile(False)
        n_out = int(yo[-1])
        bytes_moved = 8.0 * (a.utts * n_in + n_out)
        ops = 2.0 * d["P"] * n_out
        km = float(np.median(kern_ms))
        xh = x_d[:n_in].cpu().numpy()
        t0 = time.perf_counter()
        ref = signal.resample_poly(xh, up, down)
        host_ms = 1e3 * (time.perf_counter() - t0)
        same = bool(np.array_equal(y_d[:len(ref)].cpu().numpy(), ref))
        out["cases"][name] = {
            "up": up, "down": down, "P": d["P"], "n_in_total": a.utts * n_in, "n_out_total": n_out,
            "kernel_ms_median": round(km, 4), "call_ms_median": round(float(np.median(call_ms)), 4),
            "kernel_ms_min": round(float(np.min(kern_ms)), 4),
            "bytes": bytes_moved, "mul_add_ops": ops,
            "hbm_floor_ms": round(1e3 * bytes_moved / HBM_BPS, 4), "fp64_floor_ms": round(1e3 * ops / FP64_OPS, 4),
            "frac_of_hbm_floor": round(1e3 * bytes_moved / HBM_BPS / km, 3),
            "frac_of_fp64_floor": round(1e3 * ops / FP64_OPS / km, 3),
            "scipy_host_ms_per_utt": round(host_ms, 3), "first_row_equals_scipy": same,
        }
        del x_d, y_d
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
