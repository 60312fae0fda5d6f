"""Exemplar-based conversion (world/exemplar.py) at the corpus sizes, on resident random rows (the kernels do
not care where their rows came from):

  wh_knn           2 001 x 128 064 and 128 064 x 128 064 rows, d = 78, K = 16: kernel time from the library's per-launch
                   event pairs (knn_tile_kernel, knn_merge_kernel), pairs per second and the share of the FP64 issue rate
                   they stand for — 3 d FP64 instructions per pair (a subtraction, a product and a sum per column) against
                   the vector ceiling tools/dtw_bench.py counts with;
  torch            the same search as chunked torch.cdist + topk in FP64, wall time, in the same run (and how many of its
                   index rows differ: its distances are not the contract's);
  wh_frame_select  64 and 1024 utterances of 2001 frames, K = 16, dy = 39: kernel time (frame_sources_kernel,
                   frame_select_kernel), frames per second, the share of the issue rate of its 3 dy K^2 instructions per frame;
  NumPy            tests/_exemplar_reference.py on one host core, measured on a slice and extrapolated;
  smoothing        on synth_utterance speakers: leave-one-out frame selection in both modes and gmm.convert_compact trained
                   on the same alignment — the ratio of the converted to the target per-coefficient variance of the static
                   track, geometric mean over the coefficients (1.0: the target's own spread; below: over-smoothing).

Medians over --calls after --warmup.  Prints one JSON line.

    python tools/exemplar_bench.py [--calls 3] [--warmup 1] [--rows 128064] [--no-smoothing]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-world_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

FP64_ISSUE_PEAK = 78.6e12 / 2  # FP64 vector instructions x lanes per second (bench.py: FP64_VECTOR_PEAK_TFLOPS)


def med(v):
    return float(np.median(v))


def timed(rt, names, fn, calls, warmup):
    """Median kernel ms per name prefix over the calls, and the last result."""
    import torch

    kern = {n: [] for n in names}
    out = None
    for i in range(warmup + calls):
        if i == warmup:
            torch.cuda.synchronize()
            rt.profile(True)
        out = fn()
        if i >= warmup:
            rec = rt.profile_collect()
            for n in names:
                kern[n].append(sum(ms for nm, ms in rec if nm.startswith(n)))
    rt.profile(False)
    return {n: med(v) for n, v in kern.items()}, out


def knn_case(rt, n_q, n_db, d, k, calls, warmup, ref_rows):
    import torch

    import _exemplar_reference as xref
    from world.exemplar import knn_device

    g = torch.Generator(device=rt.device).manual_seed(2)
    db = torch.randn((n_db, d), generator=g, device=rt.device, dtype=torch.float64)
    q = torch.randn((n_q, d), generator=g, device=rt.device, dtype=torch.float64)
    ms, (idx, dist) = timed(rt, ("knn_tile_kernel", "knn_merge_kernel"), lambda: knn_device(rt, q, db, k), calls, warmup)
    kernel_ms = sum(ms.values())
    res = {"n_q": n_q, "n_db": n_db, "d": d, "k": k, "tile_kernel_ms": ms["knn_tile_kernel"], "merge_kernel_ms": ms["knn_merge_kernel"],
           "kernel_ms": kernel_ms, "pairs": n_q * n_db, "pairs_per_s": n_q * n_db / kernel_ms * 1e3}
    res["fp64_issue_frac"] = res["pairs_per_s"] * 3 * d / FP64_ISSUE_PEAK
    res["ceiling_ms"] = n_q * n_db * 3 * d / FP64_ISSUE_PEAK * 1e3
    # torch: chunks of queries whose distance block stays under 2 GiB
    chunk = max(1, min(n_q, (1 << 31) // (8 * n_db)))
    torch.cuda.synchronize()
    walls = []
    for _ in range(2):
        t0 = time.perf_counter()
        parts = [torch.topk(torch.cdist(q[i:i + chunk], db), k, dim=1, largest=False).indices for i in range(0, n_q, chunk)]
        t_idx = torch.cat(parts)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    res["torch_cdist_topk_ms"] = min(walls)
    res["torch_chunk_rows"] = chunk
    res["torch_rows_with_other_indices"] = int((t_idx != idx.to(torch.int64)).any(dim=1).sum())
    # the NumPy reference on one host core: a slice of the queries, extrapolated
    qs, dbs = q[:ref_rows].cpu().numpy(), db.cpu().numpy()
    t0 = time.perf_counter()
    r_idx, r_dist = xref.knn(qs, dbs, k)
    sl = time.perf_counter() - t0
    res["numpy_slice_rows"] = int(len(qs))
    res["numpy_slice_s"] = sl
    res["numpy_one_core_s_extrapolated"] = sl * n_q / len(qs)
    res["slice_equals_reference"] = bool(np.array_equal(r_idx, idx[:ref_rows].cpu().numpy())
                                         and r_dist.tobytes() == dist[:ref_rows].cpu().numpy().tobytes())
    del db, q, idx, dist, parts, t_idx
    torch.cuda.empty_cache()
    return res


def select_case(rt, n_utt, frames, n_db, k, dy, calls, warmup):
    import torch

    import _exemplar_reference as xref
    from world.exemplar import select_device

    g = torch.Generator(device=rt.device).manual_seed(3)
    off = np.arange(n_utt + 1, dtype=np.int64) * frames
    batch = rt.make_batch(np.zeros(n_utt + 1, dtype=np.int64), off)
    y = torch.randn((n_db, 2 * dy), generator=g, device=rt.device, dtype=torch.float64)
    idx = torch.randint(0, n_db, (n_utt * frames, k), generator=g, device=rt.device, dtype=torch.int32)
    tc = torch.rand((n_utt * frames, k), generator=g, device=rt.device, dtype=torch.float64) * dy
    succ = torch.clamp(torch.arange(1, n_db + 1, device=rt.device, dtype=torch.int32), max=n_db - 1)
    ms, out = timed(rt, ("frame_sources_kernel", "frame_select_kernel"), lambda: select_device(rt, batch, idx, tc, y[:, :dy], succ, 1.0),
                    calls, warmup)
    kernel_ms = sum(ms.values())
    n = n_utt * frames
    res = {"utterances": n_utt, "frames": frames, "k": k, "dy": dy, "n_db": n_db, "sources_kernel_ms": ms["frame_sources_kernel"],
           "select_kernel_ms": ms["frame_select_kernel"], "kernel_ms": kernel_ms, "frames_per_s": n / kernel_ms * 1e3,
           "us_per_frame_of_an_utterance": ms["frame_select_kernel"] * 1e3 / frames}
    res["fp64_issue_frac"] = res["frames_per_s"] * 3 * dy * k * k / FP64_ISSUE_PEAK
    f = 200  # the NumPy reference on one host core: the first 200 frames of utterance 0, extrapolated
    t0 = time.perf_counter()
    r_sel, _, _, r_acc = xref.frame_select([0, f], idx[:f].cpu().numpy(), tc[:f].cpu().numpy(), y[:, :dy].cpu().numpy(),
                                           succ.cpu().numpy(), 1.0)
    sl = time.perf_counter() - t0
    res["numpy_slice_frames"] = f
    res["numpy_slice_s"] = sl
    res["numpy_one_core_s_extrapolated"] = sl * n / f
    del y, idx, tc, out
    torch.cuda.empty_cache()
    return res


def smoothing(n_utt=12, seconds=1.0, n0=25, k=16, components=4):
    """Variance ratios of the converted static track, leave-one-out frame selection against the GMM."""
    import torch

    from world import exemplar, gmm
    from world._synthetic import synth_utterance
    from world.batch import WorldBatch

    fs = 16000
    wb = WorldBatch(0)
    enc_a = wb.encode([synth_utterance(300 + u, fs, seconds) for u in range(n_utt)], fs, f0_method="dio", want_coarse=True)
    enc_b = wb.encode([synth_utterance(400 + u, fs, seconds) for u in range(n_utt)], fs, f0_method="dio", want_coarse=True)
    ce_a, ce_b = enc_a.compact(n0=n0), enc_b.compact(n0=n0)
    al = ce_a.align(ce_b)
    db = exemplar.build_compact(ce_a, ce_b, al)
    model, _ = gmm.fit_compact(ce_a, ce_b, al, components, n_iter=10, reg_covar=1e-4)
    target_var = torch.var(ce_b.mcep[:, 1:], dim=0, unbiased=False)

    def ratio(ce):
        r = torch.var(ce.mcep[:, 1:], dim=0, unbiased=False) / target_var
        return float(torch.exp(torch.log(r).mean()))

    loo = list(range(n_utt))
    out = {"utterances": n_utt, "seconds": seconds, "n0": n0, "k": k, "gmm_components": components, "frames": int(ce_a.total_frames),
           "database_rows": db.n_rows, "source": ratio(ce_a),
           "frames_leave_one_out": ratio(exemplar.convert_compact(ce_a, db, k=k, mode="frames", exclude=loo)[0]),
           "mlpg_leave_one_out": ratio(exemplar.convert_compact(ce_a, db, k=k, mode="mlpg", exclude=loo)[0]),
           "gmm_mlpg": ratio(gmm.convert_compact(ce_a, model)), "gmm_mmse": ratio(gmm.convert_compact(ce_a, model, mode="mmse"))}
    out["flags"] = wb.rt.take_flags()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", type=int, default=128064)
    ap.add_argument("--queries", default="2001,128064")
    ap.add_argument("--utts", default="64,1024")
    ap.add_argument("--no-smoothing", action="store_true")
    args = ap.parse_args()
    from world import _hip

    rt = _hip.Runtime.get()
    res = {"tool": "exemplar_bench", "abi": int(rt.lib.wh_version()), "knn": [], "frame_select": []}
    for n_q in (int(v) for v in args.queries.split(",") if v):
        res["knn"].append(knn_case(rt, n_q, args.rows, 78, 16, args.calls, args.warmup, 16))
    for n_utt in (int(v) for v in args.utts.split(",") if v):
        res["frame_select"].append(select_case(rt, n_utt, 2001, args.rows, 16, 39, args.calls, args.warmup))
    if not args.no_smoothing:
        res["smoothing_variance_ratio"] = smoothing()
    res["flags"] = rt.take_flags()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
