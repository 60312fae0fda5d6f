"""Joint-density Gaussian mixture voice conversion (Toda, Black and Tokuda 2007): the model between align() /
dynamic_features() on one side and mlpg_device() on the other.  A mixture with full covariances is fitted by EM on the
joint rows [x; y] of two aligned speakers; a source row is converted by the posterior over the components under the
marginal of x, the conditional mean and variance of y given x for the most likely component, and MLPG over the result.

The frame-proportional work — the whitening product of the E-step, the weighted outer-product sums of the statistics,
the affine map of the conversion — runs on the FP64 matrix cores behind wh_gmm_estep / wh_gmm_stats / wh_gmm_convert
(csrc/wh_gmm.hip; contract in include/world_hip.h, DESIGN section 16, and in NumPy in tests/_gmm_reference.py).  The
per-component algebra (a d x d Cholesky factor per component, its inverse, the regression matrices) is tiny and is NumPy
on the host.  Neither scipy nor scikit-learn is imported.

The argument checks, the tables and the workspace grouping are host code and need neither the library nor a GPU."""
import numpy as np

from . import _hip
from .dynamics import HTS_WINDOWS, check_windows

# the kernels' limits and tiling (csrc/wh_gmm.hip: kGmmMaxD, kGmmMaxM, kGmmRowTile, kGmmSplitRows); the tests put their
# shapes around the last two, and tests/test_gmm_host.py holds the two files together
MAX_D = 160
MAX_M = 64
ROW_TILE = 128
SPLIT_ROWS = 4096
DEFAULT_MAX_WORKSPACE_BYTES = 4 << 30
CONVERT_MODES = ("mlpg", "mmse", "frame")
CONVERSION_WINDOWS = HTS_WINDOWS[:2]  # static + delta: 39 + 39 coefficients per speaker, a joint vector of 156


# ---- host ------------------------------------------------------------------------------------------------------------
def check_limits(d, m, where="gmm"):
    if not 1 <= int(d) <= MAX_D:
        raise ValueError("%s: rows of %d columns; the kernels take 1 .. %d" % (where, d, MAX_D))
    if not 1 <= int(m) <= MAX_M:
        raise ValueError("%s: %d components; the kernels take 1 .. %d" % (where, m, MAX_M))


def workspace_bytes(n_rows, d, m):
    """What wh_gmm_stats takes of the context's scratch for ``n_rows`` rows: one (d + 1) x (d + 1) partial result per
    component and run of SPLIT_ROWS rows (3.2 GB for 2 049 024 rows, d = 156, M = 32)."""
    check_limits(d, m, "workspace_bytes")
    if n_rows < 0:
        raise ValueError("workspace_bytes: n_rows must be >= 0")
    return 8 * ((int(n_rows) + SPLIT_ROWS - 1) // SPLIT_ROWS) * int(m) * (int(d) + 1) ** 2


def plan_row_groups(n_rows, d, m, max_workspace_bytes=DEFAULT_MAX_WORKSPACE_BYTES):
    """Consecutive row ranges [r0, r1) per wh_gmm_stats call: as many whole runs of SPLIT_ROWS rows as keep the partial
    results under ``max_workspace_bytes``, at least one run."""
    per_run = workspace_bytes(SPLIT_ROWS, d, m)
    rows = max(1, int(max_workspace_bytes) // per_run) * SPLIT_ROWS
    return [(r0, min(int(n_rows), r0 + rows)) for r0 in range(0, int(n_rows), rows)]


def cholesky_tables(weights, means, covariances, where="gmm"):
    """(whiten [M][d][d], logc [M]) of a mixture: L_m by numpy.linalg.cholesky, W_m = L_m^-T by substitution (upper
    triangular, the lower triangle zeros), logc[m] = log w_m - sum log diag L_m - (d / 2) log 2 pi.  ValueError naming the
    component whose covariance is not symmetric positive definite."""
    w, mu, cov = (np.asarray(a, dtype=np.float64) for a in (weights, means, covariances))
    m, d = mu.shape
    whiten, logc = np.zeros((m, d, d)), np.zeros(m)
    for k in range(m):
        if not np.all(np.isfinite(cov[k])) or not np.array_equal(cov[k], cov[k].T):
            raise ValueError("%s: the covariance of component %d is not symmetric and finite" % (where, k))
        try:
            low = np.linalg.cholesky(cov[k])
        except np.linalg.LinAlgError:
            raise ValueError("%s: the covariance of component %d is not positive definite" % (where, k))
        inv = np.zeros((d, d))  # L^-1, row by row: L inv = I
        for i in range(d):
            row = -(low[i, :i] @ inv[:i])
            row[i] += 1.0
            inv[i] = row / low[i, i]
        whiten[k] = np.triu(inv.T)
        logc[k] = np.log(w[k]) - np.sum(np.log(np.diag(low))) - 0.5 * d * np.log(2.0 * np.pi)
    return whiten, logc


def m_step(means, s0, s1, s2, reg_covar):
    """The host M-step from statistics centred at ``means``: nk = s0 + 10 eps, delta = s1 / nk, mu += delta,
    Sigma = s2 / nk - delta delta' + reg_covar I, w = nk / sum nk.  Returns (weights, means, covariances)."""
    nk = np.asarray(s0, dtype=np.float64) + 10.0 * np.finfo(np.float64).eps
    delta = s1 / nk[:, None]
    d = means.shape[1]
    cov = s2 / nk[:, None, None] - delta[:, :, None] * delta[:, None, :] + reg_covar * np.eye(d)[None]
    return nk / np.sum(nk), means + delta, cov


class JointGMM:
    """A mixture over joint rows [x; y]: weights [M], means [M][D], covariances [M][D][D] (host float64), the first
    ``dx`` columns being the source's.  ``kind`` says what the rows are made of: 'mcep' (mel-cepstral coefficients
    1 .. n0-1) or 'lsf' (the ``lsf_order`` angles of line spectral frequencies); for 'lsf', ``lsf_min_gap`` is the
    smallest of w_1, pi - w_p and any adjacent gap over the target's training rows — the default repair of a conversion,
    which is then never sharper than anything the target speaker produced.  A model does not know the sampling rate of
    the rows it was fitted on: angles of the same order from another rate are converted without complaint (they mean other
    frequencies), so keep a model with the corpus it came from."""

    def __init__(self, weights, means, covariances, dx, kind="mcep", lsf_order=None, lsf_min_gap=None):
        if kind not in ("mcep", "lsf"):
            raise ValueError("JointGMM: kind must be 'mcep' or 'lsf', got %r" % (kind,))
        if (kind == "lsf") != (lsf_order is not None) or (kind == "lsf") != (lsf_min_gap is not None):
            raise ValueError("JointGMM: lsf_order and lsf_min_gap belong to kind 'lsf' and to no other")
        self.kind = kind
        self.lsf_order = None if lsf_order is None else int(lsf_order)
        self.lsf_min_gap = None if lsf_min_gap is None else float(lsf_min_gap)
        self.weights = np.ascontiguousarray(weights, dtype=np.float64)
        self.means = np.ascontiguousarray(means, dtype=np.float64)
        self.covariances = np.ascontiguousarray(covariances, dtype=np.float64)
        if self.means.ndim != 2:
            raise ValueError("JointGMM: means must be [M][D], got shape %s" % (self.means.shape,))
        m, d = self.means.shape
        check_limits(d, m, "JointGMM")
        if self.weights.shape != (m,) or self.covariances.shape != (m, d, d):
            raise ValueError("JointGMM: weights must be [%d] and covariances [%d][%d][%d], got %s and %s"
                             % (m, m, d, d, self.weights.shape, self.covariances.shape))
        if isinstance(dx, bool) or int(dx) != dx or not 1 <= dx <= d - 1:
            raise ValueError("JointGMM: dx must be an integer in [1, %d], got %r" % (d - 1, dx))
        if not np.all(self.weights > 0.0) or not np.all(np.isfinite(self.weights)) or not np.all(np.isfinite(self.means)):
            raise ValueError("JointGMM: weights must be positive and finite, means finite")
        self.dx = int(dx)
        self._host = None
        self._dev = {}
        self.host_tables()  # (raises for a covariance that is not symmetric positive definite)

    n_components = property(lambda self: self.means.shape[0])
    dim = property(lambda self: self.means.shape[1])
    dy = property(lambda self: self.means.shape[1] - self.dx)

    def marginal_x(self):
        """(weights, means [M][dx], covariances [M][dx][dx]) of the source columns."""
        dx = self.dx
        return self.weights, np.ascontiguousarray(self.means[:, :dx]), np.ascontiguousarray(self.covariances[:, :dx, :dx])

    def host_tables(self):
        """The tables the kernels take, NumPy: 'whiten' / 'logc' of the joint mixture, 'whiten_x' / 'logc_x' of the
        marginal of x, 'a' [M][dx][dy] = Sigma_xx^-1 Sigma_xy, 'mu_x', 'mu_y', and 'cvar' [M][dy], the diagonal of
        Sigma_yy - Sigma_yx Sigma_xx^-1 Sigma_xy."""
        if self._host is None:
            dx = self.dx
            whiten, logc = cholesky_tables(self.weights, self.means, self.covariances, "JointGMM")
            wx, mux, cxx = self.marginal_x()
            whiten_x, logc_x = cholesky_tables(wx, mux, cxx, "JointGMM")
            cxy = self.covariances[:, :dx, dx:]
            half = np.einsum("mki,mkj->mij", whiten_x, cxy)  # W_x' Sigma_xy = L_x^-1 Sigma_xy
            a = np.einsum("mik,mkj->mij", whiten_x, half)
            cvar = np.einsum("mii->mi", self.covariances[:, dx:, dx:]) - np.sum(half * half, axis=1)
            self._host = {"whiten": whiten, "logc": logc, "whiten_x": whiten_x, "logc_x": logc_x,
                          "a": np.ascontiguousarray(a), "mu_x": mux, "mu_y": np.ascontiguousarray(self.means[:, dx:]),
                          "cvar": np.ascontiguousarray(cvar), "mu": self.means}
        return self._host

    def prepared(self, rt):
        """host_tables() resident on ``rt``'s device (uploaded once per runtime)."""
        key = (rt.index, rt.lane)
        if key not in self._dev:
            with rt.lock, rt.on_stream():
                self._dev[key] = {k: rt.to_device(v) for k, v in self.host_tables().items()}
        return self._dev[key]

    def save_npz(self, path):
        out = {"weights": self.weights, "means": self.means, "covariances": self.covariances, "dx": np.asarray(self.dx)}
        if self.kind == "lsf":  # (a file without the keys is a mel-cepstral model: files written before load as they did)
            out.update(kind=np.asarray("lsf"), lsf_order=np.asarray(self.lsf_order), lsf_min_gap=np.asarray(self.lsf_min_gap))
        np.savez(path, **out)

    @classmethod
    def load_npz(cls, path):
        with np.load(path) as z:
            if "kind" not in z.files:
                return cls(z["weights"], z["means"], z["covariances"], int(z["dx"]))
            return cls(z["weights"], z["means"], z["covariances"], int(z["dx"]), str(z["kind"]), int(z["lsf_order"]),
                       float(z["lsf_min_gap"]))


def check_convert_args(x_shape, frames, gmm, mode, windows, where="convert"):
    """ValueError for what convert_device cannot take.  Returns (win, half, d_y): the windows and the static columns of
    the target."""
    if mode not in CONVERT_MODES:
        raise ValueError("%s: mode must be one of %s, got %r" % (where, CONVERT_MODES, mode))
    win, half = check_windows(windows, where)
    if len(x_shape) != 2 or int(x_shape[0]) != frames:
        raise ValueError("%s: x must be [%d frames][%d], got %s" % (where, frames, gmm.dx, tuple(x_shape)))
    n_win = len(win)
    if int(x_shape[1]) != gmm.dx or gmm.dx % n_win or gmm.dy % n_win:
        raise ValueError("%s: rows of %d columns and a model of %d + %d columns do not hold %d windows each"
                         % (where, int(x_shape[1]), gmm.dx, gmm.dy, n_win))
    return win, half, gmm.dy // n_win


# ---- device: the three entries on tensors ----------------------------------------------------------------------------
def _rows(rt, name, t, width, where):
    if t.dim() != 2 or t.dtype != rt.torch.float64 or t.stride(1) != 1 or (width is not None and int(t.shape[1]) != width):
        raise ValueError("%s: %s must be a float64 [rows][%s] tensor with unit column stride, got %s %s strides %s"
                         % (where, name, "d" if width is None else width, t.dtype, tuple(t.shape), tuple(t.stride())))
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


def estep_device(rt, x, mu, whiten, logc, want=("gamma", "rowll", "best")):
    """wh_gmm_estep on device tensors: x [n][d] (row stride free), mu [M][d], whiten [M][d][d], logc [M] (contiguous).
    Returns a dict of the outputs named in ``want`` ('ll', 'gamma', 'rowll', 'best')."""
    m, d = int(mu.shape[0]), int(mu.shape[1])
    check_limits(d, m, "estep")
    ldx = _rows(rt, "x", x, d, "estep")
    n = int(x.shape[0])
    with rt.lock, rt.on_stream():
        out = {k: rt.empty((n, m)) for k in ("ll", "gamma") if k in want}
        if "rowll" in want:
            out["rowll"] = rt.empty((n,))
        if "best" in want:
            out["best"] = rt.empty((n,), rt.torch.int32)
        _hip.check(rt.lib.wh_gmm_estep(rt.ctx, rt.stream(), rt.ptr(x), n, ldx, d, m, rt.ptr(mu), rt.ptr(whiten), rt.ptr(logc),
                                       rt.ptr(out.get("ll")), m, rt.ptr(out.get("gamma")), m, rt.ptr(out.get("rowll")),
                                       rt.ptr(out.get("best"))))
    return out


def stats_device(rt, x, gamma, mu, max_workspace_bytes=DEFAULT_MAX_WORKSPACE_BYTES):
    """wh_gmm_stats on device tensors, the rows handed over in the groups of plan_row_groups and the groups' results
    added on the device in group order: (s0 [M], s1 [M][d], s2 [M][d][d])."""
    m, d = int(mu.shape[0]), int(mu.shape[1])
    check_limits(d, m, "stats")
    ldx, ldg = _rows(rt, "x", x, d, "stats"), _rows(rt, "gamma", gamma, m, "stats")
    n = int(x.shape[0])
    if int(gamma.shape[0]) != n:
        raise ValueError("stats: %d rows of x against %d of gamma" % (n, int(gamma.shape[0])))
    with rt.lock, rt.on_stream():
        total = None
        for r0, r1 in plan_row_groups(n, d, m, max_workspace_bytes):
            part = (rt.empty((m,)), rt.empty((m, d)), rt.empty((m, d, d)))
            _hip.check(rt.lib.wh_gmm_stats(rt.ctx, rt.stream(), rt.ptr(x[r0:r1]), r1 - r0, ldx, d, m, rt.ptr(gamma[r0:r1]), ldg,
                                           rt.ptr(mu), rt.ptr(part[0]), rt.ptr(part[1]), rt.ptr(part[2])))
            if total is None:
                total = part
            else:
                for t, p in zip(total, part):
                    t += p
        if total is None:
            total = (rt.zeros((m,)), rt.zeros((m, d)), rt.zeros((m, d, d)))
    return total


def convert_rows_device(rt, x, mu_x, a, mu_y, best=None, g=None):
    """wh_gmm_convert on device tensors: out [n][dy]."""
    m, dx, dy = int(a.shape[0]), int(a.shape[1]), int(a.shape[2])
    check_limits(dx + dy, m, "convert")
    if (best is None) == (g is None):
        raise ValueError("convert: exactly one of best and g must be given")
    ldx = _rows(rt, "x", x, dx, "convert")
    ldg = _rows(rt, "g", g, m, "convert") if g is not None else 0
    n = int(x.shape[0])
    with rt.lock, rt.on_stream():
        out = rt.empty((n, dy))
        _hip.check(rt.lib.wh_gmm_convert(rt.ctx, rt.stream(), rt.ptr(x), n, ldx, dx, dy, m, rt.ptr(mu_x), rt.ptr(a),
                                         rt.ptr(mu_y), rt.ptr(best), rt.ptr(g), ldg, rt.ptr(out), dy))
    return out


# ---- device: the model -----------------------------------------------------------------------------------------------
def posteriors_device(rt, x, gmm):
    """(gamma [n][M], rowll [n], best [n] int32) of rows x under ``gmm``: under the joint mixture for rows of D columns,
    under the marginal of x for rows of dx columns."""
    t = gmm.prepared(rt)
    if x.dim() == 2 and int(x.shape[1]) == gmm.dx:
        o = estep_device(rt, x, t["mu_x"], t["whiten_x"], t["logc_x"])
    elif x.dim() == 2 and int(x.shape[1]) == gmm.dim:
        o = estep_device(rt, x, t["mu"], t["whiten"], t["logc"])
    else:
        raise ValueError("posteriors: x must be [rows][%d] (the source columns) or [rows][%d] (joint rows), got %s"
                         % (gmm.dx, gmm.dim, tuple(x.shape)))
    return o["gamma"], o["rowll"], o["best"]


def fit_device(rt, z, dx, n_components, n_iter, reg_covar=1e-6, init=None, seed=0,
               max_workspace_bytes=DEFAULT_MAX_WORKSPACE_BYTES):
    """EM with full covariances on the joint rows z [n][D] (float64 device tensor): (JointGMM, history), history[i] the
    mean log-likelihood per row under the parameters iteration i started from.  ``init``: a JointGMM, or None — every
    choice made on the host from numpy.random.default_rng(seed): the means are ``n_components`` distinct rows of z, every
    covariance the global covariance + reg_covar I, the weights equal.  One iteration is wh_gmm_estep (gamma and rowll),
    wh_gmm_stats centred at the current means, a download of s0, s1, s2 and m_step on the host."""
    if z.dim() != 2:
        raise ValueError("fit: z must be [rows][D], got shape %s" % (tuple(z.shape),))
    n, d = int(z.shape[0]), int(z.shape[1])
    m = int(n_components)
    check_limits(d, m, "fit")
    if isinstance(dx, bool) or int(dx) != dx or not 1 <= dx <= d - 1:
        raise ValueError("fit: dx must be an integer in [1, %d], got %r" % (d - 1, dx))
    if n < m or n < 2:
        raise ValueError("fit: %d rows for %d components" % (n, m))
    if int(n_iter) < 0 or not reg_covar >= 0.0:
        raise ValueError("fit: n_iter and reg_covar must be >= 0")
    _rows(rt, "z", z, d, "fit")
    torch = rt.torch
    with rt.lock, rt.on_stream():
        if init is not None:
            if init.dim != d or init.n_components != m or init.dx != dx:
                raise ValueError("fit: init is a model of %d components over %d + %d columns" % (init.n_components, init.dx, init.dy))
            w, mu, cov = init.weights, init.means, init.covariances
        else:
            rng = np.random.default_rng(seed)
            pick = np.sort(rng.choice(n, size=m, replace=False))
            mu = z.index_select(0, torch.from_numpy(pick).to(rt.device)).cpu().numpy()
            centre = rt.to_device(mu[:1])
            s0, s1, s2 = (t.cpu().numpy() for t in stats_device(rt, z, rt.torch.ones((n, 1), dtype=torch.float64, device=rt.device),
                                                                centre, max_workspace_bytes))
            delta = s1[0] / s0[0]
            glob = s2[0] / s0[0] - np.outer(delta, delta) + reg_covar * np.eye(d)
            w, cov = np.full(m, 1.0 / m), np.repeat(glob[None], m, axis=0)
        history = []
        for _ in range(int(n_iter)):
            whiten, logc = cholesky_tables(w, mu, cov, "fit")
            mu_d = rt.to_device(mu)
            o = estep_device(rt, z, mu_d, rt.to_device(whiten), rt.to_device(logc), want=("gamma", "rowll"))
            s0, s1, s2 = stats_device(rt, z, o["gamma"], mu_d, max_workspace_bytes)
            history.append(float(o["rowll"].sum().item()) / n)
            w, mu, cov = m_step(mu, s0.cpu().numpy(), s1.cpu().numpy(), s2.cpu().numpy(), reg_covar)
    return JointGMM(w, mu, cov, dx), history


def convert_device(rt, batch, x, gmm, mode="mlpg", windows=CONVERSION_WINDOWS):
    """Source rows x [F][n_win d] (static then dynamic columns, as delta_features_device lays them out; the frames of
    ``batch``) -> the target's static track [F][d_y].  'mlpg': the most likely component under the marginal of x, its
    conditional mean rows and conditional variances, and mlpg_device over them.  'mmse': the posterior-weighted
    conditional mean of the static columns.  'frame': the most likely component's conditional mean, static columns."""
    from .dynamics import mlpg_device

    win, _, d_y = check_convert_args(tuple(x.shape), batch.total_frames, gmm, mode, windows)
    t = gmm.prepared(rt)
    with rt.lock, rt.on_stream():
        o = estep_device(rt, x, t["mu_x"], t["whiten_x"], t["logc_x"], want=("gamma",) if mode == "mmse" else ("best",))
        if mode == "mlpg":
            mean = convert_rows_device(rt, x, t["mu_x"], t["a"], t["mu_y"], best=o["best"])
            var = rt.torch.index_select(t["cvar"], 0, o["best"].to(rt.torch.int64))
            return mlpg_device(rt, batch, mean, var, windows)
        if "a_static" not in t:  # the static columns' tables, contiguous
            t["a_static"] = t["a"][:, :, :d_y].contiguous()
            t["mu_y_static"] = t["mu_y"][:, :d_y].contiguous()
        if mode == "mmse":
            return convert_rows_device(rt, x, t["mu_x"], t["a_static"], t["mu_y_static"], g=o["gamma"])
        return convert_rows_device(rt, x, t["mu_x"], t["a_static"], t["mu_y_static"], best=o["best"])


# ---- mel-cepstra: CompactEncoding and the NumPy-dict forms ------------------------------------------------------------
def _frames_batch(rt, frame_off):
    return rt.make_batch(np.zeros(len(frame_off), dtype=np.int64), frame_off)


def fit_mceps(rt, batch_a, mcep_a, batch_b, mcep_b, alignment, n_components, n_iter=20, windows=CONVERSION_WINDOWS, **fit_kw):
    """fit_device on the two speakers' static + dynamic rows of mel-cepstral coefficients 1 .. n0-1, gathered through
    ``alignment.joint``."""
    from .dynamics import delta_features_device

    check_windows(windows, "fit_conversion")
    if mcep_a.shape[1] != mcep_b.shape[1] or int(mcep_a.shape[1]) < 2:
        raise ValueError("fit_conversion: mel-cepstra of %d and %d coefficients" % (mcep_a.shape[1], mcep_b.shape[1]))
    width = len(windows) * (int(mcep_a.shape[1]) - 1)
    check_limits(2 * width, n_components, "fit_conversion")
    with rt.lock, rt.on_stream():
        fa = delta_features_device(rt, batch_a, mcep_a[:, 1:], windows)
        fb = delta_features_device(rt, batch_b, mcep_b[:, 1:], windows)
        z, _ = alignment.joint(fa, fb)
        return fit_device(rt, z, width, n_components, n_iter, **fit_kw)


def fit_compact(ce_a, ce_b, alignment, n_components, n_iter=20, windows=CONVERSION_WINDOWS, **fit_kw):
    """(JointGMM, history) for two resident CompactEncodings of parallel utterances and their Alignment: the static +
    delta rows of both speakers without coefficient 0, joined along the alignment's paths, and fit_device."""
    for ce in (ce_a, ce_b):
        if ce.rt is None or (ce.mcep is None and ce.lsf is None):
            raise ValueError("fit_compact: the encodings must be resident (to_device(rt)) and hold a mel-cepstrum or line "
                             "spectral frequencies")
    if ce_a.kind != ce_b.kind or ce_a.lsf_order != ce_b.lsf_order:
        raise ValueError("fit_compact: the two encodings differ in kind or order (%r %r against %r %r)"
                         % (ce_a.kind, ce_a.lsf_order, ce_b.kind, ce_b.lsf_order))
    if ce_a.lsf is not None and ce_a.fs != ce_b.fs:
        raise ValueError("fit_compact: sampling rates differ (%r, %r): the angles would not be comparable" % (ce_a.fs, ce_b.fs))
    if ce_a.rt is not ce_b.rt:
        raise ValueError("fit_compact: the two encodings live on different runtimes (device / lane)")
    rt = ce_a.rt
    if ce_a.total_frames != alignment.batch_a.total_frames or ce_b.total_frames != alignment.batch_b.total_frames:
        raise ValueError("fit_compact: the alignment was not made from these encodings (%d and %d frames against %d and %d)"
                         % (ce_a.total_frames, ce_b.total_frames, alignment.batch_a.total_frames, alignment.batch_b.total_frames))
    if ce_a.lsf is not None:
        check_lsf_width(ce_a.lsf_order, windows, "fit_compact")
    with rt.lock, rt.on_stream():
        if ce_a.lsf is not None:
            return fit_lsf(rt, _frames_batch(rt, ce_a.frame_off), ce_a.lsf, _frames_batch(rt, ce_b.frame_off), ce_b.lsf,
                           alignment, n_components, n_iter, windows, **fit_kw)
        return fit_mceps(rt, _frames_batch(rt, ce_a.frame_off), ce_a.mcep, _frames_batch(rt, ce_b.frame_off), ce_b.mcep,
                         alignment, n_components, n_iter, windows, **fit_kw)


# ---- line spectral frequencies: the same chain over the p angles, at any sampling rate ----------------------------------
def check_lsf_width(p, windows, where="fit_conversion"):
    """ValueError for an order whose joint rows the kernels do not take: n_win p columns per speaker, 2 n_win p <= 160
    (p <= 40 with CONVERSION_WINDOWS)."""
    n_win = len(windows)
    if 2 * n_win * int(p) > MAX_D:
        raise ValueError("%s: line spectral frequencies of order %d with %d windows give joint rows of %d columns; the "
                         "kernels take at most %d columns (order <= %d)" % (where, p, n_win, 2 * n_win * int(p), MAX_D,
                                                                           MAX_D // (2 * n_win)))


def lsf_min_gap(rows):
    """The smallest of w_1, pi - w_p and any adjacent gap over rows [F][p + 1] = [log E, w_1 .. w_p] (a torch tensor or
    a NumPy array): how sharp the sharpest envelope of these rows is, as a host float.  Each term is one rounded
    subtraction; a NaN anywhere gives NaN."""
    w = rows[:, 1:]
    parts = [float(w[:, 0].min()), float((float(np.pi) - w[:, -1]).min()), float((w[:, 1:] - w[:, :-1]).min())]
    return float("nan") if any(v != v for v in parts) else min(parts)


def fit_lsf(rt, batch_a, lsf_a, batch_b, lsf_b, alignment, n_components, n_iter=20, windows=CONVERSION_WINDOWS, **fit_kw):
    """fit_mceps over rows [log E, w_1 .. w_p]: the gain is dropped as coefficient 0 is, the model is marked 'lsf' and
    keeps the target's smallest gap."""
    p = int(lsf_a.shape[1]) - 1
    check_lsf_width(p, windows)
    gap = lsf_min_gap(lsf_b)
    if not (gap > 0.0 and np.isfinite(gap)):
        raise ValueError("fit_conversion: the target's line spectral frequencies are not strictly ascending inside "
                         "(0, pi) (smallest gap %r)" % gap)
    model, history = fit_mceps(rt, batch_a, lsf_a, batch_b, lsf_b, alignment, n_components, n_iter, windows, **fit_kw)
    return JointGMM(model.weights, model.means, model.covariances, model.dx, "lsf", p, gap), history


def convert_lsf(rt, batch, lsf, gmm, mode="mlpg", windows=CONVERSION_WINDOWS, min_gap=None):
    """Rows [F][p + 1] -> the converted rows: the angles through convert_device, then repaired (``min_gap``: the model's
    lsf_min_gap when None); log E carried over."""
    from .lsf import repair_device

    if gmm.kind != "lsf" or gmm.lsf_order != int(lsf.shape[1]) - 1:
        raise ValueError("convert: rows of line spectral frequencies of order %d against a model of kind %r, order %r"
                         % (int(lsf.shape[1]) - 1, gmm.kind, gmm.lsf_order))
    with rt.lock, rt.on_stream():
        rows = convert_mcep(rt, batch, lsf, gmm, mode, windows)
        repair_device(rt, rows[:, 1:], gmm.lsf_min_gap if min_gap is None else min_gap, out=rows[:, 1:])
    return rows


def convert_mcep(rt, batch, mcep, gmm, mode="mlpg", windows=CONVERSION_WINDOWS):
    """Mel-cepstrum [F][n0] -> the converted one: columns 1 .. n0-1 through convert_device, column 0 carried over."""
    from .dynamics import delta_features_device

    win, _ = check_windows(windows, "convert")
    d = int(mcep.shape[1]) - 1
    if d < 1 or len(win) * d != gmm.dx or gmm.dy != gmm.dx:
        raise ValueError("convert: a mel-cepstrum of %d coefficients and %d windows against a model of %d + %d columns"
                         % (d + 1, len(win), gmm.dx, gmm.dy))
    with rt.lock, rt.on_stream():
        x = delta_features_device(rt, batch, mcep[:, 1:], windows)
        y = convert_device(rt, batch, x, gmm, mode, windows)
        return rt.torch.cat([mcep[:, :1], y], dim=1)


def convert_compact(ce, gmm, windows=CONVERSION_WINDOWS, mode="mlpg", min_gap=None):
    """A new CompactEncoding whose mel-cepstral columns 1 .. n0-1 are the conversion of ``ce``'s; coefficient 0, f0, vuv,
    band aperiodicity, the voicing gate and the frame times are carried over: ready for expand(wb) -> decode_device.
    An encoding of line spectral frequencies (and a model fitted on such) converts the p angles, log E carried over, and
    ends with the repair (``min_gap``: the model's lsf_min_gap when None)."""
    if ce.rt is None:
        raise ValueError("convert_compact: the encoding is on the host; to_device(rt) first")
    if ce.mcep is None and ce.lsf is None:
        raise ValueError("convert_compact: the encoding keeps the dense spectrogram (compact(n0=None)): no mel-cepstrum")
    if ce.kind != gmm.kind or ce.lsf_order != gmm.lsf_order:
        raise ValueError("convert_compact: an encoding of kind %r, order %r against a model of kind %r, order %r"
                         % (ce.kind, ce.lsf_order, gmm.kind, gmm.lsf_order))
    rt = ce.rt
    with rt.lock, rt.on_stream():
        arrays = dict(ce._tensors())
        if ce.lsf is not None:
            arrays["lsf"] = convert_lsf(rt, _frames_batch(rt, ce.frame_off), ce.lsf, gmm, mode, windows, min_gap)
            return ce._like(rt, arrays, None if ce.tp_host is None else np.array(ce.tp_host))
        arrays["mcep"] = convert_mcep(rt, _frames_batch(rt, ce.frame_off), ce.mcep, gmm, mode, windows)
    return ce._like(rt, arrays, None if ce.tp_host is None else np.array(ce.tp_host))


def convert_waveform(wb, batch, x_d, ce, model, windows=CONVERSION_WINDOWS, mode="mlpg", min_gap=None, hop=None):
    """Vocoder-free conversion: convert_compact(ce, model), then the recording ``x_d`` of ``batch`` (WorldBatch.upload's
    pair, the waveforms ``ce`` was encoded from) filtered by the converted over the source envelope, both as coded — the
    coding error cancels in the ratio, excitation, phase and aperiodicity stay the recording's
    (world.specfilter.differential_device).  Returns (y_d in x's layout, the converted CompactEncoding).  The f0 stays the
    recording's: to move it to the target speaker's first, world.psola.modify_device(.., pitch=world.tsm.log_f0_ratio(a, b))
    leaves the formants in place (world.tsm.shift_pitch_device moves them with f0)."""
    from .specfilter import differential_device

    converted = convert_compact(ce, model, windows, mode, min_gap)
    return differential_device(wb, batch, x_d, ce, converted, hop=hop), converted


def convert_waveform_dict(fs, x, dat, model, mode="mlpg", lowhz=0, highhz=8000, windows=CONVERSION_WINDOWS):
    """World.convert_waveform: the recording ``x`` that ``dat`` was encoded from, filtered by the converted over the source
    envelope under ``model`` (both through the model's code: mel-cepstrum or line spectral frequencies): a NumPy array
    like x."""
    from .batch import BatchEncoding
    from .specfilter import _lsf_cosine_rows, filter_device

    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim != 1:
        raise ValueError("convert_waveform: x must be 1-D, got shape %s" % (x.shape,))
    if dat['fs'] != fs:
        raise ValueError("convert_waveform: the dict was encoded at %r Hz, not at fs = %r" % (dat['fs'], fs))
    win, _ = check_windows(windows, "convert_waveform")
    if model.dx % len(win) or model.dx != model.dy:
        raise ValueError("convert_waveform: a model of %d + %d columns does not hold %d windows per speaker"
                         % (model.dx, model.dy, len(win)))
    tp = np.asarray(dat['temporal_positions'], dtype=np.float64)
    frame_period = round(float(tp[1] - tp[0]) * 1e9) / 1e6 if len(tp) > 1 else 5.0
    fft_size = 2 * (int(np.shape(dat['spectrogram'])[0]) - 1)
    rt = _hip.Runtime.get()
    with rt.lock, rt.on_stream():
        enc = BatchEncoding.from_dicts(rt, [dat])
        x_d = rt.to_device(x)
        if model.kind == "lsf":
            from .lsf import lsf_device
            rows = lsf_device(rt, enc.spectrogram, model.lsf_order)
            conv = convert_lsf(rt, enc.batch, rows, model, mode, windows)
            y = filter_device(rt, x_d, [0, len(x)], fs, frame_period, fft_size, _lsf_cosine_rows(rt, conv),
                              _lsf_cosine_rows(rt, rows), kind="lsf")
        else:
            from .compact import check_compact_args
            from .features import imcep_device
            n0 = model.dx // len(win) + 1
            check_compact_args(dat['fs'], fft_size, n0, "convert_waveform")
            mc = enc.mcep(n0, lowhz, highhz)
            conv = convert_mcep(rt, enc.batch, mc, model, mode, windows)
            y = filter_device(rt, x_d, [0, len(x)], fs, frame_period, fft_size, imcep_device(rt, conv, fft_size),
                              imcep_device(rt, mc, fft_size))
        out = y.cpu().numpy()
    rt.check_flags("convert_waveform")
    return out


def _fit_conversion_lsf(dats_a, dats_b, n_components, lsf_order, n_iter, radius, windows, fit_kw):
    from .align import align_device
    from .batch import BatchEncoding
    from .lsf import check_order, lsf_device

    rates = {d['fs'] for d in dats_a} | {d['fs'] for d in dats_b}
    if len(rates) != 1:
        raise ValueError("fit_conversion: sampling rates differ (%s): the rows would not be comparable" % sorted(rates))
    p = check_order(lsf_order, "fit_conversion")
    check_lsf_width(p, windows)
    check_limits(2 * len(windows) * p, n_components, "fit_conversion")
    rt = _hip.Runtime.get()
    with rt.lock, rt.on_stream():
        enc_a, enc_b = BatchEncoding.from_dicts(rt, dats_a), BatchEncoding.from_dicts(rt, dats_b)
        la, lb = lsf_device(rt, enc_a.spectrogram, p), lsf_device(rt, enc_b.spectrogram, p)
        al = align_device(rt, enc_a.batch, la[:, 1:], enc_b.batch, lb[:, 1:], radius)
        model, _ = fit_lsf(rt, enc_a.batch, la, enc_b.batch, lb, al, n_components, n_iter, windows, **fit_kw)
    rt.check_flags("fit_conversion")
    return model


def fit_conversion_dicts(dats_a, dats_b, n_components=8, n0=40, n_iter=20, lowhz=0, highhz=8000, radius=None,
                         windows=CONVERSION_WINDOWS, lsf_order=None, **fit_kw):
    """World.fit_conversion: align the pairs, fit, return the JointGMM.  ``lsf_order``: over line spectral frequencies of
    that order instead of the mel-cepstrum, at any sampling rate."""
    from .align import align_encodings
    from .batch import BatchEncoding

    dats_a, dats_b = list(dats_a), list(dats_b)
    if len(dats_a) != len(dats_b) or not dats_a:
        raise ValueError("fit_conversion: %d dict(s) against %d: pair u is dict u of each side" % (len(dats_a), len(dats_b)))
    check_windows(windows, "fit_conversion")
    if lsf_order is not None:
        return _fit_conversion_lsf(dats_a, dats_b, n_components, lsf_order, n_iter, radius, windows, fit_kw)
    if int(n0) != n0 or n0 < 2:
        raise ValueError("fit_conversion: n0 must be an integer >= 2, got %r" % (n0,))
    check_limits(2 * len(windows) * (int(n0) - 1), n_components, "fit_conversion")
    rt = _hip.Runtime.get()
    with rt.lock, rt.on_stream():
        enc_a, enc_b = BatchEncoding.from_dicts(rt, dats_a), BatchEncoding.from_dicts(rt, dats_b)
        al = align_encodings(enc_a, enc_b, n0, lowhz, highhz, radius)
        model, _ = fit_mceps(rt, enc_a.batch, enc_a.mcep(n0, lowhz, highhz), enc_b.batch, enc_b.mcep(n0, lowhz, highhz), al,
                             n_components, n_iter, windows, **fit_kw)
    return model


def convert_voice_dict(dat, model, mode="mlpg", lowhz=0, highhz=8000, windows=CONVERSION_WINDOWS):
    """World.convert_voice: a new dict like ``dat`` whose 'spectrogram' is decode_mcep of the converted mel-cepstrum."""
    from .batch import BatchEncoding
    from .compact import check_compact_args
    from .features import imcep_device

    win, _ = check_windows(windows, "convert_voice")
    if model.dx % len(win) or model.dx != model.dy:
        raise ValueError("convert_voice: a model of %d + %d columns does not hold %d windows per speaker"
                         % (model.dx, model.dy, len(win)))
    n0 = model.dx // len(win) + 1
    fft_size = 2 * (int(np.shape(dat['spectrogram'])[0]) - 1)
    if model.kind == "lsf":  # at any sampling rate: the spectrogram is ilsf of the converted rows
        from .lsf import ilsf_device, lsf_device
        rt = _hip.Runtime.get()
        with rt.lock, rt.on_stream():
            enc = BatchEncoding.from_dicts(rt, [dat])
            rows = convert_lsf(rt, enc.batch, lsf_device(rt, enc.spectrogram, model.lsf_order), model, mode, windows)
            spec = rt.to_host(ilsf_device(rt, rows, fft_size), transpose=True)
        rt.check_flags("convert_voice")
        out = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in dict(dat).items() if k != 'out'}
        out['spectrogram'] = np.ascontiguousarray(spec)
        return out
    check_compact_args(dat['fs'], fft_size, n0, "convert_voice")
    rt = _hip.Runtime.get()
    with rt.lock, rt.on_stream():
        enc = BatchEncoding.from_dicts(rt, [dat])
        mc = convert_mcep(rt, enc.batch, enc.mcep(n0, lowhz, highhz), model, mode, windows)
        spec = rt.to_host(imcep_device(rt, mc, fft_size), transpose=True)
    rt.check_flags("convert_voice")
    out = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in dict(dat).items() if k != 'out'}
    out['spectrogram'] = np.ascontiguousarray(spec)
    return out
