"""The reference of tests/test_hip_feature_matmul.py and tests/test_feature_tables_host.py (plain NumPy, no GPU):
the product of csrc/wh_features.hip,

    out[f][n] = epi( sum_k pro(A[f][k], k) * W[k][n] ),

in np.longdouble, a forward-error bound for an FP64 evaluation of it that is DERIVED (below), not measured, a comparator
that names the worst element, a float64 emulation with the mutations the comparator must reject, and the shapes and the
data both test files run.

    prologue 0: a                          epilogue 0: acc
    prologue 1: pscale * (a * P[k])^2      epilogue 1: log(acc == 0 ? eps : acc)
    prologue 2: log a                      epilogue 2: exp(acc)
                                           epilogue 3: sqrt(max(0, acc))

An 80-bit x86 long double is assumed (eps 1.08e-19), as in tests/_fft_reference.py: a long-double sum of 1025 products is
within 1025 * 2^-64 * S of the real one, 2000 times under the FP64 bound it judges.

The bound.  u = 2^-53, S[f][n] = sum_k |pro(a_fk)| |w_kn| with the exact prologue values.

  * The sum.  Every FP64 evaluation of a sum of ka products — any order, any blocking, products rounded on their own or
    fused into the addition as the matrix cores do — is within gamma_ka * S of the exact sum of the SAME terms,
    gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1: each term
    meets at most ka roundings, each (1 + d), |d| <= u).  With ka <= 1025, gamma_ka < ka * u * (1 + 2e-13).
  * The prologue.  The terms the kernel sums are not the exact ones: prologue 1 rounds three times (a * P, its square,
    pscale times that: (1 + d1)^2 (1 + d2) (1 + d3), under 4.01 u relative), prologue 2 is the kernels' own log, held
    below 5e-16 < 5 u relative by tests/test_hip_math.py, prologue 0 is exact.  So each term carries a relative error of
    at most 5 u, which moves the sum by at most 5 u * S.
  * Together, with 3 u of slack for the second-order terms and gamma's denominator:

        |acc_fp64 - acc| <= B = (ka + 8) * u * S.

  * The epilogue, to first order in B:
      0  none: the stored value is acc_fp64 itself, and comparing it with the exact acc ROUNDED to FP64 adds that
         rounding:                                   B + u |acc|
      1  log: d log(x) = dx / x, and the kernels' log is within 5e-16 relative of the real one:
                                                     B / |acc| + 5e-16 |log acc|       (acc == 0: eps in its place)
      2  exp: exp(x + d) = exp(x) (1 + d + ...), the kernels' exp within 5e-16 relative:
                                                     exp(acc) * (B + 5e-16)
      3  sqrt of the positive part: d sqrt(x) = dx / (2 sqrt x) while the error is small against x, and one rounding
         of the (correctly rounded) square root:     B / (2 sqrt acc) + u sqrt acc     where acc > 4 B
         and where acc <= 4 B (around and below zero) both sides lie in [0, sqrt(acc + B)] <= sqrt(5 B); the two
         differ by less than sqrt(max(acc, 0) + B) - sqrt(max(acc - B, 0)) <= sqrt(2 B):
                                                     sqrt(2 B)                          otherwise.
         An acc below -B is negative in FP64 too, so the output there is exactly 0.0: the test asserts that on its own.
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, (
    "tests/_feature_reference.py needs an extended-precision np.longdouble (x86 80-bit, eps 1.08e-19); here eps is %g"
    % np.finfo(LD).eps)

U = 2.0 ** -53
EPS = 2.220446049250313e-16  # np.finfo(float).eps: what epilogue 1 puts in the place of a zero sum
FN_REL = 5e-16               # log / exp of csrc/wh_math.h, asserted in tests/test_hip_math.py

PROLOGUES, EPILOGUES = (0, 1, 2), (0, 1, 2, 3)


def _rows(A, ka, lda):
    """The (n_rows, ka) block the kernel reads of a row-major buffer with row stride lda."""
    A = np.asarray(A)
    if A.ndim == 1:
        n_rows = (len(A) - ka) // lda + 1
        A = np.lib.stride_tricks.as_strided(A, (n_rows, ka), (lda * A.itemsize, A.itemsize))
    return A[:, :ka]


def _ld_matmul(a, w):
    """a @ w in long double (einsum's loop is three times faster than matmul's for this type; the order of the sum is of
    no account at 2^-64)."""
    return np.einsum("fk,kn->fn", a, w)


def ref_product(A, ka, lda, P, pscale, W, pro, epi):
    """(acc, out, S) in np.longdouble: the exact accumulator, the exact output and S[f][n] = sum_k |pro(a_fk)| |w_kn|."""
    a = _rows(A, ka, lda).astype(LD)
    w = np.asarray(W).astype(LD)
    assert w.shape[0] == ka, (w.shape, ka)
    if pro == 1:
        v = a * np.asarray(P, dtype=np.float64)[:ka].astype(LD)
        a = LD(pscale) * (v * v)
    elif pro == 2:
        a = np.log(a)
    else:
        assert pro == 0
    acc = _ld_matmul(a, w)
    S = _ld_matmul(np.abs(a), np.abs(w))
    if epi == 0:
        out = acc.copy()
    elif epi == 1:
        out = np.log(np.where(acc == 0, LD(EPS), acc))
    elif epi == 2:
        out = np.exp(acc)
    else:
        assert epi == 3
        out = np.sqrt(np.maximum(LD(0), acc))
    return acc, out, S


def bound(acc, S, ka, epi):
    """The derived bound on |FP64 kernel output - exact output| (module docstring), elementwise, in float64."""
    acc = np.asarray(acc, dtype=LD)
    B = (LD(ka + 8) * LD(U)) * np.asarray(S, dtype=LD)
    if epi == 0:
        b = B + LD(U) * np.abs(acc)
    elif epi == 1:
        x = np.where(acc == 0, LD(EPS), acc)
        b = B / np.abs(x) + LD(FN_REL) * np.abs(np.log(np.abs(x)))
    elif epi == 2:
        b = np.exp(acc) * (B + LD(FN_REL))
    else:
        assert epi == 3
        big = acc > 4 * B
        root = np.sqrt(np.where(big, acc, LD(1)))
        b = np.where(big, B / (2 * root) + LD(U) * root, np.sqrt(2 * B))
    return b.astype(np.float64)


def compare(got, out, bnd):
    """(worst error / bound, (row, column)) of an FP64 result against the exact output.  An element that is not finite
    where the exact one is, or differs at a zero bound, counts as infinitely far out."""
    got = np.asarray(got, dtype=np.float64)
    out = np.asarray(out, dtype=LD)
    assert got.shape == out.shape == np.shape(bnd), (got.shape, out.shape, np.shape(bnd))
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got.astype(LD) - out).astype(np.float64)
        ratio = np.where(err == 0, 0.0, err / bnd)
    ratio[~np.isfinite(got) & np.isfinite(out.astype(np.float64))] = np.inf
    ratio[np.isnan(ratio)] = np.inf
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[at]), tuple(int(i) for i in at)


def check(what, got, A, ka, lda, P, pscale, W, pro, epi):
    """Compare, print the worst ratio, assert it is at most 1 with the place in the message.  Returns the ratio."""
    acc, out, S = ref_product(A, ka, lda, P, pscale, W, pro, epi)
    worst, (f, n) = compare(got, out, bound(acc, S, ka, epi))
    print("%s pro %d epi %d (%d x %d x %d): worst error / bound %.3g at row %d column %d"
          % (what, pro, epi, out.shape[0], ka, out.shape[1], worst, f, n))
    assert worst <= 1.0, (
        "%s: prologue %d epilogue %d, n_rows %d ka %d nw %d: error / bound = %.3g at row %d column %d (got %r, exact %r)"
        % (what, pro, epi, out.shape[0], ka, out.shape[1], worst, f, n, float(np.asarray(got)[f, n]), float(out[f, n])))
    return worst


def emulate(A, ka, lda, P, pscale, W, pro, epi, mutation=None):
    """The product as a plain float64 np.dot with the kernel's prologue / epilogue arithmetic: what a correct FP64
    kernel may return.  ``mutation`` makes it wrong the way a kernel could be:
      ("term", f, k)   one k term of row f dropped           ("strip", s)   the 16-wide k strip s dropped
      ("column", n)    output column n holds column n + 1     ("rows", f)    rows f and f + 16 swapped
      ("no_eps",)      epilogue 1 without the 0 -> eps substitution"""
    a = _rows(A, ka, lda).astype(np.float64)
    w = np.array(W, dtype=np.float64)
    if pro == 1:
        v = a * np.asarray(P, dtype=np.float64)[:ka]
        a = pscale * (v * v)
    elif pro == 2:
        a = np.log(a)
    kind = mutation[0] if mutation else None
    if kind == "term":
        a = a.copy()
        a[mutation[1], mutation[2]] = 0.0
    elif kind == "strip":
        a = a.copy()
        a[:, 16 * mutation[1]:16 * mutation[1] + 16] = 0.0
    acc = np.dot(a, w)
    with np.errstate(divide="ignore", invalid="ignore"):
        if epi == 1:
            out = np.log(acc if kind == "no_eps" else np.where(acc == 0, EPS, acc))
        elif epi == 2:
            out = np.exp(acc)
        elif epi == 3:
            out = np.sqrt(np.maximum(0.0, acc))
        else:
            out = acc
    if kind == "column":
        out = out.copy()
        out[:, mutation[1]] = out[:, mutation[1] + 1]
    elif kind == "rows":
        out = out.copy()
        out[[mutation[1], mutation[1] + 16]] = out[[mutation[1] + 16, mutation[1]]]
    return out


# ---- the shapes of tests/test_hip_feature_matmul.py: (n_rows, ka, nw) --------------------------------------------------
CENTRE = (129, 33, 65)
N_ROWS = (1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 257, 300)
KA = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 513, 1025)
NW = (1, 15, 16, 17, 48, 63, 64, 65, 80, 127, 128, 129, 326)
SWIPE_CORNER = (300, 1025, 326)
PAIR_SHAPES = (CENTRE, (40, 513, 20))
STRIDE_SHAPES = (CENTRE, (1, 1, 1), (17, 513, 12))
TAGGED_SECOND = (17, 17, 20)  # the second table of the tagged-tables test: another shape under another tag


def star_shapes():
    """The centre, then one dimension varied at a time (the centre once)."""
    out = [CENTRE]
    out += [(r, CENTRE[1], CENTRE[2]) for r in N_ROWS if r != CENTRE[0]]
    out += [(CENTRE[0], k, CENTRE[2]) for k in KA if k != CENTRE[1]]
    out += [(CENTRE[0], CENTRE[1], n) for n in NW if n != CENTRE[2]]
    return out


def random_shapes(count=20, seed=20):
    rng = np.random.RandomState(seed)
    return [(int(rng.choice(N_ROWS)), int(rng.choice(KA)), int(rng.choice(NW))) for _ in range(count)]


def exact_shapes():
    """Every shape of the integer-exactness test: the star, twenty seeded random triples, SWIPE's corner once."""
    return star_shapes() + random_shapes() + [SWIPE_CORNER]


def all_shapes():
    """Every (n_rows, ka, nw) the GPU test hands to the kernel directly, each once."""
    seen, out = set(), []
    for s in exact_shapes() + list(PAIR_SHAPES) + list(STRIDE_SHAPES) + [(300,) + CENTRE[1:], (1,) + CENTRE[1:], TAGGED_SECOND]:
        if s not in seen:
            seen.add(s)
            out.append(s)
    return out


def integer_data(shape, seed=0):
    """A and W of integers in [-8, 8]: |sum| <= 64 * 1025 < 2^53 and every partial sum is an integer, so FP64 is exact in
    any order.  Returns (A, W, the int64 product)."""
    n_rows, ka, nw = shape
    rng = np.random.RandomState(seed + 7919 * n_rows + 104729 * ka + 1299709 * nw)
    a = rng.randint(-8, 9, size=(n_rows, ka))
    w = rng.randint(-8, 9, size=(ka, nw))
    return a.astype(np.float64), w.astype(np.float64), a.astype(np.int64) @ w.astype(np.int64)


def pair_data(shape, pro, epi, seed=0):
    """Random data that suits a prologue / epilogue pair: (A, P, pscale, W).
      prologue 2 (log): positive magnitudes in e^[-12, 3] — e^[0.01, 3] in front of epilogue 1, whose sum of
                  non-negative weights must stay positive for its log;
      prologue 1: magnitudes in e^[-6, 3], a per-column table in [0.03, 1.97] (|1 - 0.97 e^-iw|), pscale 1 / 1024;
      prologue 0: mixed signs — non-negative in front of epilogue 1;
      epilogue 1: a non-negative W with all-zero columns (every third one), so the 0 -> eps substitution runs;
      epilogue 2: W scaled so that the arguments of exp stay within +-30;
      epilogue 3 (and 0): mixed signs in W, so some sums are negative."""
    n_rows, ka, nw = shape
    rng = np.random.RandomState(1000 * pro + 100 * epi + seed + ka)
    P, pscale = None, 1.0
    if pro == 2:
        A = np.exp(rng.uniform(0.01 if epi == 1 else -12.0, 3.0, size=(n_rows, ka)))
    elif pro == 1:
        A = np.exp(rng.uniform(-6.0, 3.0, size=(n_rows, ka)))
        P = rng.uniform(0.03, 1.97, size=ka)
        pscale = 1.0 / 1024
    else:
        A = rng.standard_normal((n_rows, ka))
        if epi == 1:
            A = np.abs(A)
    if epi == 1:
        W = rng.uniform(0.0, 1.0, size=(ka, nw)) * (rng.uniform(size=(ka, nw)) < 0.7)
        W[:, ::3] = 0.0
    else:
        W = rng.standard_normal((ka, nw))
    if epi == 2:
        W *= 29.9 / np.max(np.abs(emulate(A, ka, ka, P, pscale, W, pro, 0)))
    return A, P, pscale, W
