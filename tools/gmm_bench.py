"""The joint-density GMM kernels (world/gmm.py) at the corpus sizes: one EM iteration — wh_gmm_estep (gamma and
rowll) and wh_gmm_stats — on 2 049 024 joint rows (1024 x 10 s of aligned paths) of D = 156 columns with M = 32 components,
the conversion (wh_gmm_convert, best component) at dx = dy = 78, and the same at 131 072 rows.  Kernel times are the
library's per-launch event pairs; medians over --calls after --warmup.  FLOP counts are the contract's arithmetic — the
E-step's triangular product N M d (d + 1), the statistics' upper triangle with s1 and s0 N M (d + 1)(d + 2), the
conversion's 2 N M dx dy (every component's product is formed) — and the rate is given as a share of the 78.6 TFLOP/s FP64
matrix peak that tools/vae_bench.py uses.  In the same run: the same arithmetic written with torch FP64 batched products
(full d x d whitening products, full outer products), chunked over rows because its N x M x D intermediate would be 82 GB at
the headline shape; and, where scikit-learn imports, one GaussianMixture iteration on one host core at the smaller size.
Prints one JSON line.

    python tools/gmm_bench.py [--calls 5] [--warmup 1] [--rows 2049024,131072] [--d 156] [--m 32] [--chunk 65536]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-world_amd"))

FP64_PEAK = 78.6e12


def med(v):
    return float(np.median(v))


def make_model(d, m, dx, seed=0):
    from world import gmm

    rng = np.random.RandomState(seed)
    cov = []
    for _ in range(m):
        q, _ = np.linalg.qr(rng.standard_normal((d, d)))
        a = (q * np.exp(rng.uniform(-1.0, 1.0, size=d))) @ q.T
        cov.append((a + a.T) / 2)
    w = rng.uniform(0.5, 1.5, size=m)
    return gmm.JointGMM(w / w.sum(), 0.3 * rng.standard_normal((m, d)), np.stack(cov), dx)


def timed(fn, calls, warmup):
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


def torch_em(z, t, chunk):
    """E-step + statistics with torch batched products, ``chunk`` rows at a time."""
    import torch

    mu, whiten, logc = t["mu"], t["whiten"], t["logc"]
    m, d = mu.shape
    s0 = torch.zeros((m,), dtype=z.dtype, device=z.device)
    s1 = torch.zeros((m, d), dtype=z.dtype, device=z.device)
    s2 = torch.zeros((m, d, d), dtype=z.dtype, device=z.device)
    total = torch.zeros((), dtype=z.dtype, device=z.device)
    for r0 in range(0, z.shape[0], chunk):
        e = z[r0:r0 + chunk].unsqueeze(0) - mu.unsqueeze(1)                 # [M][c][d]
        ll = logc.unsqueeze(1) - 0.5 * torch.bmm(e, whiten).square_().sum(2)  # [M][c]
        row = torch.logsumexp(ll, dim=0)
        g = torch.exp(ll - row)
        total += row.sum()
        s0 += g.sum(1)
        s1 += torch.bmm(g.unsqueeze(1), e).squeeze(1)
        s2 += torch.bmm((e * g.unsqueeze(2)).transpose(1, 2), e)
    return s0, s1, s2, total


def torch_convert(x, t, best, chunk):
    import torch

    out = torch.empty((x.shape[0], t["a"].shape[2]), dtype=x.dtype, device=x.device)
    for r0 in range(0, x.shape[0], chunk):
        e = x[r0:r0 + chunk].unsqueeze(0) - t["mu_x"].unsqueeze(1)
        v = t["mu_y"].unsqueeze(1) + torch.bmm(e, t["a"])                    # [M][c][dy]
        idx = best[r0:r0 + chunk].to(torch.int64).view(1, -1, 1).expand(1, -1, v.shape[2])
        out[r0:r0 + chunk] = torch.gather(v, 0, idx)[0]
    return out


def case(rt, n, model, calls, warmup, chunk):
    import torch

    from world import gmm

    d, m, dx = model.dim, model.n_components, model.dx
    dy = d - dx
    g = torch.Generator(device=rt.device).manual_seed(1)
    z = torch.randn((n, d), generator=g, device=rt.device, dtype=torch.float64)
    t = model.prepared(rt)
    x = z[:, :dx]
    best = torch.randint(0, m, (n,), generator=g, device=rt.device, dtype=torch.int32)
    kern = {"gmm_estep_kernel": [], "gmm_stats_kernel": [], "gmm_combine_kernel": [], "gmm_convert_kernel": []}
    for i in range(warmup + calls):
        if i == warmup:
            torch.cuda.synchronize()
            rt.profile(True)
        o = gmm.estep_device(rt, z, t["mu"], t["whiten"], t["logc"], want=("gamma", "rowll"))
        s = gmm.stats_device(rt, z, o["gamma"], t["mu"])
        y = gmm.convert_rows_device(rt, x, t["mu_x"], t["a"], t["mu_y"], best=best)
        if i >= warmup:
            rec = rt.profile_collect()
            for name in kern:
                kern[name].append(sum(ms for nm, ms in rec if nm.startswith(name)))
    rt.profile(False)
    # the torch formulation, and how far the two agree
    ts = torch_em(z, t, chunk)
    agree = {"s2_max_rel": float(((s[2] - ts[2]).abs().max() / ts[2].abs().max()).cpu()),
             "mean_rowll_abs": float((o["rowll"].sum() / n - ts[3] / n).abs().cpu()),
             "convert_max_abs": float((y - torch_convert(x, t, best, chunk)).abs().max().cpu())}
    torch_em_ms = timed(lambda: torch_em(z, t, chunk), calls, warmup)
    torch_cv_ms = timed(lambda: torch_convert(x, t, best, chunk), calls, warmup)
    fl_e, fl_s, fl_c = n * m * d * (d + 1), n * m * (d + 1) * (d + 2), 2 * n * m * dx * dy
    e_ms, s_ms, c_ms = med(kern["gmm_estep_kernel"]), med(kern["gmm_stats_kernel"]), med(kern["gmm_convert_kernel"])
    share = lambda fl, ms: round(fl / ms / 1e9 / (FP64_PEAK / 1e12), 4)  # noqa: E731
    res = {"rows": n, "d": d, "M": m, "dx": dx, "dy": dy, "workspace_bytes": gmm.workspace_bytes(n, d, m),
           "groups": len(gmm.plan_row_groups(n, d, m)),
           "estep_kernel_ms": e_ms, "stats_kernel_ms": s_ms, "combine_kernel_ms": med(kern["gmm_combine_kernel"]),
           "em_iteration_kernels_ms": e_ms + s_ms + med(kern["gmm_combine_kernel"]), "convert_kernel_ms": c_ms,
           "estep_tflops": round(fl_e / e_ms / 1e9, 2), "estep_frac_of_fp64_peak": share(fl_e, e_ms),
           "stats_tflops": round(fl_s / s_ms / 1e9, 2), "stats_frac_of_fp64_peak": share(fl_s, s_ms),
           "convert_tflops": round(fl_c / c_ms / 1e9, 2), "convert_frac_of_fp64_peak": share(fl_c, c_ms),
           "torch_em_iteration_ms": torch_em_ms, "torch_convert_ms": torch_cv_ms, "torch_chunk_rows": chunk,
           "torch_intermediate_bytes_unchunked": 8 * n * m * d, "torch_intermediate_bytes_per_chunk": 8 * min(n, chunk) * m * d,
           "torch_em_over_kernels": torch_em_ms / (e_ms + s_ms + med(kern["gmm_combine_kernel"])),
           "torch_convert_over_kernel": torch_cv_ms / c_ms, "agreement_with_torch": agree}
    del z, o, s, y, ts
    torch.cuda.empty_cache()
    return res


def sklearn_iteration(n, model):
    """Seconds of one GaussianMixture EM iteration (E-step + M-step) on one host core, or None."""
    try:
        from sklearn.mixture import GaussianMixture
        from threadpoolctl import threadpool_limits
    except Exception:
        return None
    import warnings

    x = np.random.RandomState(1).standard_normal((n, model.dim))
    gm = GaussianMixture(n_components=model.n_components, covariance_type="full", max_iter=1, tol=0.0, reg_covar=1e-6,
                         weights_init=model.weights, means_init=model.means,
                         precisions_init=np.linalg.inv(model.covariances))
    with threadpool_limits(limits=1), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gm._initialize_parameters(x, np.random.RandomState(0))
        t0 = time.perf_counter()
        _, resp = gm._e_step(x)
        gm._m_step(x, resp)
        return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", default="2049024,131072")
    ap.add_argument("--d", type=int, default=156)
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--no-sklearn", action="store_true")
    a = ap.parse_args()
    from world import _hip

    rt = _hip.Runtime.get(0)
    model = make_model(a.d, a.m, a.d // 2)
    rows = [int(v) for v in a.rows.split(",")]
    out = {"calls": a.calls, "fp64_matrix_peak_tflops": FP64_PEAK / 1e12, "cases": {}}
    for n in rows:
        out["cases"]["%dx%dx%d" % (n, a.d, a.m)] = case(rt, n, model, a.calls, a.warmup, a.chunk)
    assert rt.take_flags() == [0] * 16
    if not a.no_sklearn:
        sec = sklearn_iteration(min(rows), model)
        out["sklearn_one_core_em_iteration_s"] = sec
        out["sklearn_rows"] = min(rows)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
