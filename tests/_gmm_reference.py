"""The contract of csrc/wh_gmm.hip and world/gmm.py in plain NumPy (no GPU), once in float64 and once in np.longdouble
(every function takes ``dtype``), the forward-error bounds the tests hold an FP64 evaluation to — DERIVED below from the
operands, never measured — and comparators that name the worst element.

    prepare      L_m (Cholesky), W_m = L_m^-T, logc[m] = log w_m - sum log diag L_m - (d/2) log 2 pi
    loglik       z = (x_n - mu_m) W_m;  ll[n][m] = logc[m] - 0.5 sum_j z_j^2
    reduce       mx = max_m ll;  s = sum_m exp(ll - mx);  rowll = mx + log s;  gamma = exp(ll - mx) / s;  best = first argmax
    stats        s0 = sum gamma;  s1 = sum gamma (x - mu);  s2 = sum gamma (x - mu)(x - mu)'
    m_step       nk = s0 + 10 eps;  delta = s1 / nk;  mu += delta;  Sigma = s2 / nk - delta delta' + reg I;  w = nk / sum nk
    conditional  A_m = Sigma_xx^-1 Sigma_xy;  cvar = diag(Sigma_yy - Sigma_yx Sigma_xx^-1 Sigma_xy)
    convert      best: mu_y[m] + (x - mu_x[m]) A_m;  mmse: sum_m g[m] (...);  mlpg: tests/_mlpg_reference.py over the best rows

An 80-bit x86 long double is assumed (eps 1.08e-19), as in tests/_feature_reference.py.

The bounds.  u = 2^-53; gamma_k = k u / (1 - k u) covers ANY order and blocking of a sum of k terms, products rounded on
their own or fused (Higham, 2nd ed., section 3.1).  F = 2 u is one ulp: the device library's exp and log are documented
to <= 1 ulp (ROCm's OCML double-precision exp / log), and these are the functions the kernel calls.

  loglik.  e_k = fl(x_k - mu_k) is within u |e_k|, so z_j as the kernel sums it is within
               Bz_j = (d + 3) u sum_k |e_k| |W_kj|
           of the exact one (gamma_d for the sum, u for e, 2 u slack for gamma's denominator and the cross terms).  Then
           |z~_j^2 - z_j^2| <= 2 |z_j| Bz_j + Bz_j^2, the squares are rounded (u) and summed over d columns in some order
           (gamma_d) — (d + 2) u sum_j (|z_j| + Bz_j)^2 — the halving is exact and the subtraction from logc rounds once:
               B_ll = 0.5 [ sum_j (2 |z_j| Bz_j + Bz_j^2) + (d + 2) u sum_j (|z_j| + Bz_j)^2 ] + u |ll|.
  reduce,  on the ll given (the device's own, so that the two stages' errors do not compound).  t_m = fl(ll_m - mx) is
           within u |t_m|, which exp turns into a relative error, plus the function's F and one u of slack:
               rp_m = u |t_m| + F + u                      (relative error of p_m = exp(t_m))
           s, a sum of M non-negative terms: rs = max_m rp_m + (M + 1) u relative.
               B_gamma = gamma (rp_m + rs + 2 u) + 1e-320   (the division rounds once; the floor covers a denormal p_m)
               B_rowll = rs + F |log s| + 2 u + u |rowll|   (d log s = ds / s; log's own F; the final addition)
           mx is the maximum of given numbers and best its first index: exact.
  stats,   per entry, T = sum_n |gamma_n| |e_ni| |e_nj| (|e_ni| alone for s1, 1 for s0): two differences (2 u), the
           product gamma e (u), n terms in some order and blocking plus the partial sums' own additions
           (gamma_(n + splits)), 3 u slack, and u |s| for comparing with the rounded exact value:
               B = (n + splits + 6) u T + u |s|.
  convert, per entry.  The kernel runs ONE accumulation over all components and k (m ascending), the mu_y terms behind
           them; T_m = sum_k |e_k| |A_kj| + |mu_y[m][j]|.
               best:  the terms of the other components are exact zeros and adding them rounds nothing; e is rounded (u),
                      dx + 1 terms are summed (gamma_(dx+1)), 2 u slack, u |out| for the rounded exact value:
                          B = (dx + 4) u T_m + u |out|,   m = best[n]
               mmse:  the operand g_m e_k is rounded twice (the difference, the product), M (dx + 1) terms are summed:
                          B = (M (dx + 1) + 5) u sum_m |g_m| T_m + u |out|.
  m_step,  on the statistics given: every entry of Sigma is a quotient, a product, a difference and a sum —
               B_Sigma = u (3 |s2 / nk| + 5 |delta_i delta_j| + 2 reg),  B_mu = u (|mu| + 3 |delta|),  B_w = (M + 3) u w.
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, (
    "tests/_gmm_reference.py needs an extended-precision np.longdouble (x86 80-bit, eps 1.08e-19); here eps is %g"
    % np.finfo(LD).eps)

U = 2.0 ** -53
F = 2.0 * U  # one ulp: the documented bound of the device library's exp and log


# ---- the contract ----------------------------------------------------------------------------------------------------
def cholesky(a, dtype=np.float64):
    """Lower triangular L with L L' = a, by columns, in ``dtype`` (numpy.linalg has no long-double form)."""
    a = np.asarray(a, dtype=dtype)
    d = a.shape[0]
    low = np.zeros((d, d), dtype=dtype)
    for j in range(d):
        s = a[j, j] - np.dot(low[j, :j], low[j, :j])
        if not s > 0:
            raise ValueError("not positive definite at column %d" % j)
        low[j, j] = np.sqrt(s)
        if j + 1 < d:
            low[j + 1:, j] = (a[j + 1:, j] - low[j + 1:, :j] @ low[j, :j]) / low[j, j]
    return low


def inv_lower(low, dtype=np.float64):
    d = low.shape[0]
    inv = np.zeros((d, d), dtype=dtype)
    for i in range(d):
        row = -(low[i, :i] @ inv[:i])
        row[i] += 1
        inv[i] = row / low[i, i]
    return inv


def prepare(w, mu, cov, dtype=np.float64, drop_logdet=False):
    """(whiten [M][d][d], logc [M]).  ``drop_logdet``: a mutant for the comparators' own tests."""
    w, mu, cov = (np.asarray(a, dtype=dtype) for a in (w, mu, cov))
    m, d = mu.shape
    whiten, logc = np.zeros((m, d, d), dtype=dtype), np.zeros(m, dtype=dtype)
    for k in range(m):
        low = cholesky(cov[k], dtype)
        whiten[k] = np.triu(inv_lower(low, dtype).T)
        logdet = np.sum(np.log(np.diag(low)))
        logc[k] = np.log(w[k]) - (0 if drop_logdet else logdet) - dtype(d) / 2 * np.log(2 * np.pi * dtype(1))
    return whiten, logc


def loglik(x, mu, whiten, logc, dtype=np.float64):
    """(ll [n][M], B_ll [n][M]) — the bound is meaningful in long double."""
    x, mu, whiten, logc = (np.asarray(a, dtype=dtype) for a in (x, mu, whiten, logc))
    n, d = x.shape
    m = mu.shape[0]
    ll, bnd = np.zeros((n, m), dtype=dtype), np.zeros((n, m), dtype=dtype)
    for k in range(m):
        e = x - mu[k]
        z = e @ whiten[k]
        bz = dtype((d + 3) * U) * (np.abs(e) @ np.abs(whiten[k]))
        ll[:, k] = logc[k] - np.sum(z * z, axis=1) / 2
        bnd[:, k] = (np.sum(2 * np.abs(z) * bz + bz * bz, axis=1) + dtype((d + 2) * U) * np.sum((np.abs(z) + bz) ** 2, axis=1)) / 2
    return ll, bnd + dtype(U) * np.abs(ll)


def reduce(ll, dtype=np.float64, normalise=True, last_max=False):
    """(gamma, rowll, best, B_gamma, B_rowll) of given ll.  ``normalise=False`` / ``last_max=True``: mutants."""
    ll = np.asarray(ll, dtype=dtype)
    n, m = ll.shape
    mx = np.max(ll, axis=1)
    best = (m - 1 - np.argmax(ll[:, ::-1], axis=1)) if last_max else np.argmax(ll, axis=1)
    t = ll - mx[:, None]
    p = np.exp(t)
    s = np.sum(p, axis=1)
    gamma = p / s[:, None] if normalise else p
    rowll = mx + np.log(s)
    rp = dtype(U) * np.abs(t) + dtype(F + U)
    rs = np.max(rp, axis=1) + dtype((m + 1) * U)
    b_gamma = gamma * (rp + rs[:, None] + dtype(2 * U)) + dtype(1e-320)
    b_rowll = rs + dtype(F) * np.abs(np.log(s)) + dtype(2 * U) + dtype(U) * np.abs(rowll)
    return gamma, rowll, best.astype(np.int32), b_gamma, b_rowll


def stats(x, gamma, mu, dtype=np.float64, splits=1, centre_shift=0):
    """(s0, s1, s2, B0, B1, B2).  ``centre_shift``: component m is centred at mu[(m + shift) % M] — a mutant."""
    x, gamma, mu = (np.asarray(a, dtype=dtype) for a in (x, gamma, mu))
    n, d = x.shape
    m = mu.shape[0]
    s0, s1, s2 = np.zeros(m, dtype=dtype), np.zeros((m, d), dtype=dtype), np.zeros((m, d, d), dtype=dtype)
    b0, b1, b2 = np.zeros(m, dtype=dtype), np.zeros((m, d), dtype=dtype), np.zeros((m, d, d), dtype=dtype)
    c = dtype((n + splits + 6) * U)
    for k in range(m):
        e = x - mu[(k + centre_shift) % m]
        g = gamma[:, k]
        s0[k], s1[k], s2[k] = np.sum(g), g @ e, (e * g[:, None]).T @ e
        ag, ae = np.abs(g), np.abs(e)
        b0[k], b1[k], b2[k] = c * np.sum(ag), c * (ag @ ae), c * ((ae * ag[:, None]).T @ ae)
    u = dtype(U)
    return s0, s1, s2, b0 + u * np.abs(s0), b1 + u * np.abs(s1), b2 + u * np.abs(s2)


def m_step(mu, s0, s1, s2, reg, dtype=np.float64):
    """(w, mu, cov, B_w, B_mu, B_cov)."""
    mu, s0, s1, s2 = (np.asarray(a, dtype=dtype) for a in (mu, s0, s1, s2))
    m, d = mu.shape
    nk = s0 + dtype(10 * np.finfo(np.float64).eps)
    delta = s1 / nk[:, None]
    q = s2 / nk[:, None, None]
    dd = delta[:, :, None] * delta[:, None, :]
    cov = q - dd + dtype(reg) * np.eye(d, dtype=dtype)[None]
    w = nk / np.sum(nk)
    new_mu = mu + delta
    u = dtype(U)
    return (w, new_mu, cov, dtype((m + 3) * U) * w, u * (np.abs(new_mu) + 3 * np.abs(delta)),
            u * (3 * np.abs(q) + 5 * np.abs(dd) + 2 * dtype(reg)))


def textbook_m_step(x, gamma, reg, dtype=LD):
    """The uncentred textbook sums: mu = sum g x / sum g, Sigma = sum g x x' / sum g - mu mu' + reg I."""
    x, gamma = np.asarray(x, dtype=dtype), np.asarray(gamma, dtype=dtype)
    nk = np.sum(gamma, axis=0) + dtype(10 * np.finfo(np.float64).eps)
    mu = (gamma.T @ x) / nk[:, None]
    d = x.shape[1]
    cov = np.stack([(x * gamma[:, k:k + 1]).T @ x / nk[k] - np.outer(mu[k], mu[k]) for k in range(gamma.shape[1])])
    return nk / np.sum(nk), mu, cov + dtype(reg) * np.eye(d, dtype=dtype)[None]


def conditional(w, mu, cov, dx, dtype=np.float64, transpose_a=False):
    """{'mu_x', 'mu_y', 'a' [M][dx][dy], 'cvar' [M][dy], 'whiten_x', 'logc_x'}.  ``transpose_a``: a mutant (dx == dy)."""
    w, mu, cov = (np.asarray(a, dtype=dtype) for a in (w, mu, cov))
    m = mu.shape[0]
    whiten_x, logc_x = prepare(w, mu[:, :dx], cov[:, :dx, :dx], dtype)
    a, cvar = [], []
    for k in range(m):
        half = whiten_x[k].T @ cov[k, :dx, dx:]
        ak = whiten_x[k] @ half
        a.append(ak.T.copy() if transpose_a else ak)
        cvar.append(np.diag(cov[k, dx:, dx:]) - np.sum(half * half, axis=0))
    return {"mu_x": mu[:, :dx].copy(), "mu_y": mu[:, dx:].copy(), "a": np.stack(a), "cvar": np.stack(cvar),
            "whiten_x": whiten_x, "logc_x": logc_x}


def component_means(x, mu_x, a, mu_y, dtype=np.float64):
    """(v [M][n][dy], T [M][n][dy]) — every component's conditional mean of every row and T_m of the bound."""
    x, mu_x, a, mu_y = (np.asarray(t, dtype=dtype) for t in (x, mu_x, a, mu_y))
    v, tm = [], []
    for k in range(a.shape[0]):
        e = x - mu_x[k]
        v.append(mu_y[k] + e @ a[k])
        tm.append(np.abs(e) @ np.abs(a[k]) + np.abs(mu_y[k]))
    return np.stack(v), np.stack(tm)


def convert_best(x, mu_x, a, mu_y, best, dtype=np.float64):
    """(out [n][dy], B)."""
    v, tm = component_means(x, mu_x, a, mu_y, dtype)
    rows = np.arange(x.shape[0])
    out = v[np.asarray(best), rows]
    return out, dtype((x.shape[1] + 4) * U) * tm[np.asarray(best), rows] + dtype(U) * np.abs(out)


def convert_mmse(x, mu_x, a, mu_y, g, dtype=np.float64):
    v, tm = component_means(x, mu_x, a, mu_y, dtype)
    g = np.asarray(g, dtype=dtype).T[:, :, None]  # [M][n][1]
    out = np.sum(g * v, axis=0)
    m = v.shape[0]
    bnd = dtype((m * (x.shape[1] + 1) + 5) * U) * np.sum(np.abs(g) * tm, axis=0)
    return out, bnd + dtype(U) * np.abs(out)


def convert(x, w, mu, cov, dx, mode, windows, lens, dtype=np.float64):
    """The three conversion modes on rows x [F][dx] of utterances of ``lens`` frames, float64 arithmetic of the contract:
    the static track [F][d_y].  'mlpg' runs tests/_mlpg_reference.py per utterance."""
    import _mlpg_reference as mref

    t = conditional(w, mu, cov, dx, dtype)
    ll, _ = loglik(x, t["mu_x"], t["whiten_x"], t["logc_x"], dtype)
    gamma, _, best, _, _ = reduce(ll, dtype)
    d_y = (mu.shape[1] - dx) // len(windows)
    if mode == "mmse":
        return convert_mmse(x, t["mu_x"], t["a"][:, :, :d_y], t["mu_y"][:, :d_y], gamma, dtype)[0]
    if mode == "frame":
        return convert_best(x, t["mu_x"], t["a"][:, :, :d_y], t["mu_y"][:, :d_y], best, dtype)[0]
    mean, _ = convert_best(x, t["mu_x"], t["a"], t["mu_y"], best, dtype)
    var = t["cvar"][best]
    off = np.concatenate([[0], np.cumsum(lens)])
    return np.concatenate([mref.mlpg(np.asarray(mean[a:b], dtype=np.float64), np.asarray(var[a:b], dtype=np.float64), windows)[0]
                           for a, b in zip(off[:-1], off[1:])])


# ---- comparison ------------------------------------------------------------------------------------------------------
def compare(got, exact, bnd):
    """(worst error / bound, index) of an FP64 result against the exact one.  An element that is not finite where the
    exact one is, or differs at a zero bound, counts as infinitely far out."""
    got = np.asarray(got, dtype=np.float64)
    exact = np.asarray(exact, dtype=LD)
    bnd = np.broadcast_to(np.asarray(bnd, dtype=LD), exact.shape)
    assert got.shape == exact.shape, (got.shape, exact.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got.astype(LD) - exact)
        ratio = np.where(err == 0, LD(0), err / bnd).astype(np.float64)
    ratio = np.atleast_1d(ratio)
    ratio[np.atleast_1d(~np.isfinite(got) & np.isfinite(exact.astype(np.float64)))] = np.inf
    ratio[np.isnan(ratio)] = np.inf
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[at]), tuple(int(i) for i in at)


WORST = {}  # what -> the worst ratio seen in this process (the tests print it; the docstrings quote it)


def check(what, got, exact, bnd):
    worst, at = compare(got, exact, bnd)
    WORST[what.split(" ")[0]] = max(WORST.get(what.split(" ")[0], 0.0), worst)
    print("%s: worst error / bound %.3g at %s" % (what, worst, at))
    assert worst <= 1.0, "%s: error / bound = %.3g at %s (got %r, exact %r)" % (
        what, worst, at, float(np.asarray(got)[at]), float(np.asarray(exact, dtype=LD)[at]))
    return worst


# ---- data --------------------------------------------------------------------------------------------------------------
def random_spd(d, cond, rng):
    """A symmetric positive definite matrix with eigenvalues log-uniform in [1 / cond, 1] and a random orthogonal basis,
    symmetric bit for bit."""
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    lam = np.exp(rng.uniform(-np.log(cond), 0.0, size=d)) if d > 1 else np.ones(1)
    if d > 1:
        lam[0], lam[-1] = 1.0, 1.0 / cond
    a = (q * lam) @ q.T
    return (a + a.T) / 2


def random_mixture(m, d, rng, cond=1e6, spread=2.0):
    """(w, mu, cov): condition numbers log-uniform up to ``cond``."""
    w = rng.uniform(0.5, 1.5, size=m)
    w /= np.sum(w)
    mu = spread * rng.standard_normal((m, d))
    cov = np.stack([random_spd(d, 10.0 ** rng.uniform(0.0, np.log10(cond)), rng) for _ in range(m)])
    return w, mu, cov


def sample(w, mu, cov, n, rng):
    """n rows drawn from the mixture."""
    k = rng.choice(len(w), size=n, p=w)
    low = np.stack([np.linalg.cholesky(c) for c in cov])
    return mu[k] + np.einsum("nij,nj->ni", low[k], rng.standard_normal((n, mu.shape[1]))), k
