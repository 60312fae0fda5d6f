"""Frame-grid conversion (world/regrid.py) at the corpus sizes: 64 x 10 s and 1024 x 10 s of resident
synthetic [F][513] tensors at 16 kHz (no encode: the kernel does not care where its rows came from), 5 -> 10 ms and
5 -> 2.5 ms.  Per case: kernel time of wh_regrid_rows (the library's per-launch event pairs: regrid_plan_kernel +
regrid_rows_kernel), a device-to-device copy_ of the OUTPUT tensor in the same run, and the algorithmic bytes of each —
the kernel reads every source row it needs once and writes every output row once, the copy reads and writes the output's
size.  The figure of merit is kernel time over copy time, set against the ratio of those bytes: (2 + 1) / (1 + 1) = 1.5
for 5 -> 10 ms counting two source rows' worth per output row (on the uniform grids every destination frame is an exact hit and
reads one: byte_ratio_counted), (0.5 + 1) / 2 = 0.75 for
5 -> 2.5 ms.  Medians over --calls after --warmup.  Prints one JSON line.

    python tools/regrid_bench.py [--calls 10] [--warmup 2] [--utts 64,1024]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-world_amd"))

FS, K, NFU = 16000, 513, 2001  # 10 s at 5 ms
BYTE_RATIO = {10: (2 + 1) / (1 + 1), 2.5: (0.5 + 1) / 2}


def med(v):
    return float(np.median(v))


def timed(torch, fn, calls, warmup):
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


def case(rt, utts, period, calls, warmup):
    import torch

    from world._tables import frame_times
    from world.regrid import destination_times, regrid_rows_device

    t_src = frame_times(NFU, 5)
    t_dst = destination_times(t_src, period)
    nd = len(t_dst)
    src = rt.make_batch(np.zeros(utts + 1, dtype=np.int64), np.arange(utts + 1, dtype=np.int64) * NFU)
    dst = rt.make_batch(np.zeros(utts + 1, dtype=np.int64), np.arange(utts + 1, dtype=np.int64) * nd)
    tp_s, tp_d = rt.to_device(np.tile(t_src, utts)), rt.to_device(np.tile(t_dst, utts))
    g = torch.Generator(device=rt.device).manual_seed(1)
    rows = torch.rand((utts * NFU, K), generator=g, device=rt.device, dtype=torch.float64).add_(0.05)
    out = rt.empty((utts * nd, K))
    kern = {"regrid_plan_kernel": [], "regrid_rows_kernel": []}
    for i in range(warmup + calls):
        if i == warmup:
            torch.cuda.synchronize()
            rt.profile(True)
        regrid_rows_device(rt, src, dst, tp_s, tp_d, rows, out=out)
        if i >= warmup:
            rec = rt.profile_collect()
            for name in kern:
                kern[name].append(sum(ms for nm, ms in rec if nm.startswith(name)))
    rt.profile(False)
    twin = torch.empty_like(out)
    copy_ms = timed(torch, lambda: twin.copy_(out), calls, warmup)
    # rows of the source the kernel needs: those np.interp reads for some destination frame
    j = np.clip(np.searchsorted(t_src, t_dst, side="right") - 1, 0, NFU - 1)
    two = (j < NFU - 1) & (t_src[j] != t_dst)
    read_rows = len(np.unique(np.concatenate([j, j[two] + 1])))
    row_b = K * 8
    kernel_ms = med(kern["regrid_plan_kernel"]) + med(kern["regrid_rows_kernel"])
    res = {"utts": utts, "src_frames": utts * NFU, "dst_frames": utts * nd, "bins": K,
           "plan_kernel_ms": med(kern["regrid_plan_kernel"]), "rows_kernel_ms": med(kern["regrid_rows_kernel"]),
           "kernel_ms": kernel_ms, "copy_of_output_ms": copy_ms,
           "kernel_bytes": utts * (read_rows + nd) * row_b + utts * nd * (8 + 2 * 32),
           "copy_bytes": 2 * utts * nd * row_b,
           "kernel_over_copy": kernel_ms / copy_ms, "byte_ratio_nominal": BYTE_RATIO[period]}
    res["byte_ratio_counted"] = res["kernel_bytes"] / res["copy_bytes"]
    res["kernel_GBps"] = res["kernel_bytes"] / kernel_ms / 1e6
    res["copy_GBps"] = res["copy_bytes"] / copy_ms / 1e6
    res["over_nominal_byte_ratio"] = res["kernel_over_copy"] / res["byte_ratio_nominal"]
    del rows, out, twin
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--utts", default="64,1024")
    a = ap.parse_args()
    from world import _hip

    rt = _hip.Runtime.get(0)
    out = {"fs": FS, "bins": K, "calls": a.calls, "cases": {}}
    for utts in (int(v) for v in a.utts.split(",")):
        for period in (10, 2.5):
            out["cases"]["%dx10s_5->%sms" % (utts, period)] = case(rt, utts, period, a.calls, a.warmup)
    assert rt.take_flags() == [0] * 16
    print(json.dumps(out))


if __name__ == "__main__":
    main()
