"""Device time of the manifold vocoder's networks (wh_dense_stack): the TIMIT encoder + decoder
(39 -> 256 -> 256 -> 256 -> 12 -> 256 -> 256 -> 256 -> 39, 288 256 multiply-adds per frame) over 2 049 024 frames of
resident 40-dim MCEP, as World.encode_vae runs them (one launch, latent as the tap, mean shift in and out).  The median
over >= 20 calls (after warm-up) of the kernel time (the library's per-launch event pairs) and of the whole call; the
rate in TFLOP/s and as a fraction of the 78.6 TFLOP/s FP64 matrix peak.  As a yardstick only: the same chain as
torch.addmm + relu in FP64 on the same data.  Prints one JSON line.

    python tools/vae_bench.py [--calls 20] [--warmup 3] [--frames 2049024]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-world_amd"))
GOLDEN = os.path.join(ROOT, "tests", "golden")

FP64_PEAK = 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=2049024)
    a = ap.parse_args()
    import torch

    from world import _hip
    from world.manifold import DenseStack, vae_device

    rt = _hip.Runtime.get()
    enc = DenseStack.from_h5(os.path.join(GOLDEN, "manifold_timit_vae_encoder.h5"))
    dec = DenseStack.from_h5(os.path.join(GOLDEN, "manifold_timit_vae_decoder.h5"))
    macs = sum(w.shape[0] * w.shape[1] for w in enc.weights + dec.weights)
    flops = 2.0 * macs * a.frames
    g = np.load(os.path.join(GOLDEN, "golden_manifold.npz"))
    mean = g["mean"]
    reps = -(-a.frames // len(g["mcep"]))
    mcep = np.tile(g["mcep"], (reps, 1))[:a.frames]
    mc_d = rt.to_device(np.ascontiguousarray(mcep))
    x_d = mc_d[:, 1:]

    def timed(fn, kernel=None):
        for _ in range(a.warmup):
            r = fn()
        torch.cuda.synchronize()
        call_ms, kern_ms = [], []
        if kernel:
            rt.profile(True)
        for _ in range(a.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn()
            e1.record()
            e1.synchronize()
            call_ms.append(e0.elapsed_time(e1))
            if kernel:
                kern_ms.append(sum(ms for nm, ms in rt.profile_collect() if nm.startswith(kernel)))
        if kernel:
            rt.profile(False)
        return r, float(np.median(call_ms)), (float(np.median(kern_ms)) if kernel else None)

    (z_d, y_d), call_ms, kern_ms = timed(lambda: vae_device(rt, x_d, enc, dec, 0, mean), "dense_stack_kernel")
    layers = [(torch.from_numpy(w.astype(np.float64)).to(rt.device), torch.from_numpy(b.astype(np.float64)).to(rt.device),
               act) for w, b, act in list(enc.layers()) + list(dec.layers())]
    mean_d = torch.from_numpy(mean).to(rt.device)

    def torch_chain():
        h = x_d - mean_d
        for i, (w, b, act) in enumerate(layers):
            h = torch.addmm(b, h, w)
            if act == "relu":
                h = torch.relu(h)
            if i == len(enc) - 1:
                h = h.float().double()
        return h + mean_d

    y_t, torch_ms, _ = timed(torch_chain)
    diff = float((y_t - y_d).abs().max().item())
    out = {
        "frames": a.frames, "calls": a.calls, "macs_per_frame": macs, "tflop": round(flops / 1e12, 4),
        "kernel_ms_median": round(kern_ms, 4), "call_ms_median": round(call_ms, 4),
        "tflops": round(flops / kern_ms / 1e9, 3), "frac_of_fp64_peak": round(flops / kern_ms / 1e9 / (FP64_PEAK / 1e12), 4),
        "fp64_floor_ms": round(1e3 * flops / FP64_PEAK, 3),
        "torch_addmm_relu_ms_median": round(torch_ms, 4), "torch_tflops": round(flops / torch_ms / 1e9, 3),
        "speedup_vs_torch": round(torch_ms / kern_ms, 3), "max_abs_diff_vs_torch": diff,
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
