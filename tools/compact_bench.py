"""Compact encodings (world/compact.py) at the corpus sizes: the 64 x 10 s config-2 batch, really encoded
(DIO path), and 1024 x 10 s = 2 049 024 frames of resident synthetic tensors (no encode: the expansion does not care
where its bands came from).  Per size: kernel time of wh_aperiodicity_from_bands (the library's per-launch event pairs)
against a device-to-device copy_ of an FP64 tensor of the output's size in the same run (the copy moves twice the
bytes), time of compact() and of expand() between stream events, bytes per frame each way (asserted: dense
(2 K + 3) * 8, compact (n0 + nap + 4) * 8).  At 64 x 10 s also the wall time of encode followed by the D2H of the
compact tensors against encode followed by the D2H of the dense ones (WorldBatch.download_async).  Medians over
--calls after --warmup.  Prints one JSON line.

    python tools/compact_bench.py [--calls 10] [--warmup 2] [--big-utts 1024]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-world_amd"))

FS, SECONDS, N0 = 16000, 10.0, 40


def med(v):
    return float(np.median(v))


def timed(torch, fn, calls, warmup):
    """Median ms of fn() between two stream events."""
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


def resident_case(wb, enc, calls, warmup):
    """Kernel, compact() and expand() times on a resident encoding that holds coarse_ap / ap_gate."""
    import torch

    from world.d4c import aperiodicity_from_bands_device

    rt = wb.rt
    nf, k = (int(v) for v in enc.aperiodicity.shape)
    nap = int(enc.coarse_ap.shape[1])
    res = {"frames": nf, "bins": k, "bands": nap}
    dense_b, compact_b = (2 * k + 3) * 8, (N0 + nap + 4) * 8
    ce = enc.compact(N0)
    assert ce.nbytes() == nf * compact_b
    assert sum(t.numel() * 8 for t in (enc.temporal_positions, enc.f0, enc.vuv, enc.spectrogram, enc.aperiodicity)) == nf * dense_b
    res["bytes_per_frame"] = {"dense": dense_b, "compact": compact_b, "ratio": dense_b / compact_b}
    res["bytes"] = {"dense": nf * dense_b, "compact": nf * compact_b}
    kern = []
    for i in range(warmup + calls):
        if i == warmup:
            torch.cuda.synchronize()
            rt.profile(True)
        ap = aperiodicity_from_bands_device(rt, enc.coarse_ap, enc.ap_gate, FS, enc.fft_size)
        if i >= warmup:
            kern.append(sum(ms for nm, ms in rt.profile_collect() if nm.startswith("ap_from_bands_kernel")))
    rt.profile(False)
    dst = torch.empty_like(ap)
    copy_ms = timed(torch, lambda: dst.copy_(ap), calls, warmup)
    del dst, ap
    res["ap_from_bands_kernel_ms"] = med(kern)
    res["copy_same_size_ms"] = copy_ms
    res["kernel_over_copy"] = med(kern) / copy_ms
    res["kernel_write_GBps"] = nf * k * 8 / med(kern) / 1e6
    res["kernel_over_copy_bound"] = 1.5
    res["compact_ms"] = timed(torch, lambda: enc.compact(N0), calls, warmup)
    res["expand_ms"] = timed(torch, lambda: ce.expand(wb), calls, warmup)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--big-utts", type=int, default=1024)
    a = ap.parse_args()
    import torch

    from world._synthetic import synth_utterance
    from world.batch import BatchEncoding, WorldBatch

    wb = WorldBatch(0)
    rt = wb.rt
    out = {"fs": FS, "n0": N0, "calls": a.calls, "cases": {}}

    # ---- 64 x 10 s, really encoded ------------------------------------------------------------------------------------
    xs = [synth_utterance(u, FS, SECONDS) for u in range(a.utts)]
    batch, x_d, tp_d = wb.upload(xs, FS)

    def encode(want_coarse):
        return wb.encode_device(batch, x_d, tp_d, FS, f0_method="dio", check=False, want_coarse=want_coarse)

    enc = encode(True)
    wb.check()
    case = resident_case(wb, enc, a.calls, a.warmup)

    def flow_compact():
        e = encode(True)
        return e.compact(N0).to_host()

    def flow_dense():
        e = encode(False)
        pins, done = wb.download_async([e.temporal_positions, e.f0, e.vuv, e.spectrogram, e.aperiodicity])
        done.synchronize()
        return pins

    def flow_resident():
        encode(False)
        torch.cuda.synchronize()

    walls = {}
    for name, fn in (("encode_resident", flow_resident), ("encode_plus_compact_d2h", flow_compact),
                     ("encode_plus_dense_d2h", flow_dense)):
        ts = []
        for i in range(a.warmup + a.calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        walls[name + "_ms"] = med(ts)
    wb.check()
    case["wall"] = walls
    case["compact_faster_than_dense"] = walls["encode_plus_compact_d2h_ms"] < walls["encode_plus_dense_d2h_ms"]
    out["cases"]["%dx%.0fs" % (a.utts, SECONDS)] = case
    del enc, x_d, tp_d
    torch.cuda.empty_cache()

    # ---- 1024 x 10 s of resident synthetic tensors ------------------------------------------------------------------
    if a.big_utts > 0:
        nfu = 2001
        nf = a.big_utts * nfu
        k = 513
        g = torch.Generator(device=rt.device).manual_seed(1)
        frame_off = np.arange(a.big_utts + 1, dtype=np.int64) * nfu
        big = rt.make_batch(np.zeros(a.big_utts + 1, dtype=np.int64), frame_off)
        tp = torch.arange(nfu, dtype=torch.float64, device=rt.device).mul_(0.005).repeat(a.big_utts)
        gate = (torch.rand(nf, generator=g, device=rt.device) > 0.3).to(torch.float64)
        coarse = torch.rand((nf, 1), generator=g, device=rt.device, dtype=torch.float64).mul_(-30.0)
        spec = torch.rand((nf, k), generator=g, device=rt.device, dtype=torch.float64).add_(0.05)
        enc = BatchEncoding(rt, big, FS, tp, gate * 120.0, gate.clone(), spec, torch.empty((nf, k), dtype=torch.float64, device=rt.device),
                            1024, False, 5)
        enc.coarse_ap, enc.ap_gate = coarse, gate
        out["cases"]["%dx%.0fs_synthetic" % (a.big_utts, SECONDS)] = resident_case(wb, enc, a.calls, a.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
