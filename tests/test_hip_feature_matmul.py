"""GPU: feature_matmul_kernel and context_kernel (csrc/wh_features.hip) called directly through the C-ABI, at the shapes
where a tiled matrix-core kernel goes wrong, against tests/_feature_reference.py (a long-double product with a derived
forward-error bound) and NumPy restatements of the reference's heads (tests/test_feature_tables_host.py).

  a  integers in [-8, 8]: every partial sum is exact in FP64, the output equals the int64 product bit for bit — a star
     around (129, 33, 65), twenty random triples, SWIPE's (300, 1025, 326);
  b  all twelve prologue x epilogue pairs against the long-double reference, within the derived bound;
  c  lda != ka, ldo != nw, NaN around A, a sentinel around and between the rows of out: nothing else read or written;
  d  a row of a 300-row call has the bits of the same row computed alone;
  e  the persistent tables follow their contents (untagged) and their tags (tagged);
  f  the three heads at D in {257, 1025, 2049} with a second column block (nfilt 65, 80; n0 65);
  g  wh_context_frames against the slicing definition.

Worst error / bound of test b per pair, MI355X, 2026-10-17, kernel as of commit 6ee078e (129 x 33 x 65 | 40 x 513 x 20):
             epilogue 0          1 (log)           2 (exp)           3 (sqrt+)
  prologue 0  0.080  | 0.0052    0.141 | 0.141     0.081 | 0.0042    0.082 | 0.0056
  prologue 1  0.184  | 0.0144    0.149 | 0.141     0.148 | 0.0123    0.162 | 0.0126
  prologue 2  0.101  | 0.0035    0.141 | 0.141     0.068 | 0.0049    0.073 | 0.0059
(0.141 is the kernels' log at eps, 1.4 ulp inside the 5e-16 it is held to; the 300 x 33 x 65 call of test d: 0.098.  A value
above 1 is a finding about the kernel, never a reason to widen the bound; np.dot on the host gives 0.003 to 0.19 on the
same data, tests/test_feature_tables_host.py)."""
import ctypes

import numpy as np
import pytest

import _feature_reference as R
from conftest import rel_rms

pytestmark = pytest.mark.gpu

_vp = ctypes.c_void_p


def _rt():
    from world import _hip

    return _hip.Runtime.get()


def _matmul(rt, a_d, n_rows, ka, lda, W, out_d, ldo, pro=0, P=None, pscale=1.0, epi=0, tag=None):
    """wh_feature_matmul (tag None) or wh_feature_matmul_tagged on device tensors / views; W and P are host arrays."""
    from world import _hip

    W = np.ascontiguousarray(W, dtype=np.float64)
    assert W.shape[0] == ka
    P = np.ascontiguousarray(P, dtype=np.float64) if P is not None else None
    pp = P.ctypes.data_as(_vp) if P is not None else _vp(None)
    args = (rt.ctx, rt.stream(), rt.ptr(a_d), int(n_rows), int(ka), int(lda), int(pro), pp, float(pscale),
            W.ctypes.data_as(_vp), int(W.shape[1]), int(epi), rt.ptr(out_d), int(ldo))
    if tag is None:
        _hip.check(rt.lib.wh_feature_matmul(*args))
    else:
        _hip.check(rt.lib.wh_feature_matmul_tagged(*args, int(tag)))


def _product(rt, A, W, pro=0, P=None, pscale=1.0, epi=0, tag=None):
    """Contiguous A (host) -> the (n_rows, nw) result on the host."""
    n_rows, ka = A.shape
    out = rt.empty((n_rows, W.shape[1]))
    _matmul(rt, rt.to_device(A), n_rows, ka, ka, W, out, W.shape[1], pro, P, pscale, epi, tag)
    return out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- a ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(enumerate(R.exact_shapes())), ids=lambda c: "%d-%dx%dx%d" % ((c[0],) + c[1]))
def test_integer_products_are_exact(case):
    shape = case[1]
    A, W, exact = R.integer_data(shape)
    got = _product(_rt(), A, W)
    assert got.shape == exact.shape
    bad = np.argwhere(_bits(got) != _bits(exact.astype(np.float64)))
    assert len(bad) == 0, "n_rows %d ka %d nw %d: %d wrong elements, the first at row %d column %d: %r for %d" % (
        shape + (len(bad), bad[0][0], bad[0][1], got[tuple(bad[0])], exact[tuple(bad[0])]))


# ---- b ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.PAIR_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("epi", R.EPILOGUES)
@pytest.mark.parametrize("pro", R.PROLOGUES)
def test_every_prologue_and_epilogue(shape, pro, epi):
    n_rows, ka, nw = shape
    A, P, pscale, W = R.pair_data(shape, pro, epi)
    got = _product(_rt(), A, W, pro, P, pscale, epi)
    assert np.all(np.isfinite(got))
    R.check("feature_matmul_kernel", got, A, ka, ka, P, pscale, W, pro, epi)
    if epi == 1:  # the all-zero columns of W: the sum is exactly 0 and eps is put in its place
        assert np.all(got[:, ::3] == got[0, 0]) and abs(got[0, 0] - np.log(R.EPS)) < 2e-14
    if epi == 3:  # sums that are negative beyond their rounding error come out as exactly 0.0
        acc, _, S = R.ref_product(A, ka, ka, P, pscale, W, pro, epi)
        neg = acc < -((ka + 8) * R.U) * S
        assert neg.any() and np.all(_bits(got[neg]) == 0)


# ---- c ---------------------------------------------------------------------------------------------------------------------
SENTINEL = 0x7FF85EA71E550BAD  # (a NaN payload no arithmetic produces)
GUARD = 64


@pytest.mark.parametrize("tagged", (False, True), ids=("untagged", "tagged"))
@pytest.mark.parametrize("shape", R.STRIDE_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_strides_and_guard_bands(shape, tagged):
    from world import _hip

    rt = _rt()
    n_rows, ka, nw = shape
    lda, ldo = ka + 7, nw + 5
    A, W, exact = R.integer_data(shape, seed=1)
    a_h = np.full(GUARD + n_rows * lda + GUARD, np.nan)
    for f in range(n_rows):
        a_h[GUARD + f * lda:GUARD + f * lda + ka] = A[f]
    a_d = rt.to_device(a_h)
    tile_rows = -(-n_rows // 128) * 128  # the rows the last workgroup's tile spans: all but n_rows of them guarded off
    out_raw = rt.torch.full((GUARD + tile_rows * ldo + GUARD,), SENTINEL, dtype=rt.torch.int64, device=rt.device)
    out_d = out_raw.view(rt.torch.float64)[GUARD:]
    _matmul(rt, a_d[GUARD:], n_rows, ka, lda, W, out_d, ldo, tag=_hip.table_tag(W) if tagged else None)
    raw = out_raw.cpu().numpy()
    assert np.all(raw[:GUARD] == SENTINEL) and np.all(raw[-GUARD:] == SENTINEL)
    body = raw[GUARD:-GUARD].reshape(tile_rows, ldo)
    written = np.zeros(body.shape, dtype=bool)
    written[:n_rows, :nw] = True
    stray = np.argwhere((body != SENTINEL) & ~written)
    assert len(stray) == 0, "%d elements written outside [f < %d][n < %d], the first at row %d column %d" % (
        len(stray), n_rows, nw, stray[0][0], stray[0][1])
    got = np.ascontiguousarray(body[:n_rows, :nw]).view(np.float64)
    assert not np.isnan(got).any()  # neither a sentinel left in place nor a NaN read from around A
    assert np.array_equal(_bits(got), _bits(exact.astype(np.float64)))
    assert np.array_equal(_bits(a_d.cpu().numpy()), _bits(a_h))


# ---- d ---------------------------------------------------------------------------------------------------------------------
def test_a_row_does_not_depend_on_its_neighbours():
    rt = _rt()
    n_rows, ka, nw = (300,) + R.CENTRE[1:]
    rng = np.random.RandomState(4)
    A, W = rng.standard_normal((n_rows, ka)), rng.standard_normal((ka, nw))
    a_d = rt.to_device(A)
    full = rt.empty((n_rows, nw))
    _matmul(rt, a_d, n_rows, ka, ka, W, full, nw)
    full = full.cpu().numpy()
    R.check("feature_matmul_kernel", full, A, ka, ka, None, 1.0, W, 0, 0)
    for f in (0, 15, 16, 127, 128, 299):
        one = rt.empty((1, nw))
        _matmul(rt, a_d[f], 1, ka, ka, W, one, nw)
        assert np.array_equal(_bits(one.cpu().numpy()[0]), _bits(full[f])), f


# ---- e ---------------------------------------------------------------------------------------------------------------------
def test_untagged_tables_follow_their_contents():
    rt = _rt()
    A, W1, exact1 = R.integer_data(R.CENTRE, seed=2)
    _, W2, _ = R.integer_data(R.CENTRE, seed=3)
    assert not np.array_equal(W1, W2)
    exact2 = A.astype(np.int64) @ W2.astype(np.int64)
    for W, exact in ((W1, exact1), (W2, exact2), (W1, exact1), (W1, exact1), (W2, exact2)):
        assert np.array_equal(_product(rt, A, W), exact.astype(np.float64))


def test_tagged_tables_follow_their_tags():
    from world import _hip

    rt = _rt()
    A1, W1, exact1 = R.integer_data(R.CENTRE, seed=4)
    A2, W2, exact2 = R.integer_data(R.TAGGED_SECOND, seed=5)
    # the same shape as W1 under another tag: the slot is keyed by tag AND shape, and by the tag alone between these two
    A3, W3, exact3 = R.integer_data(R.CENTRE, seed=6)
    t1, t2, t3 = _hip.table_tag(W1), _hip.table_tag(W2), _hip.table_tag(W3)
    assert len({t1, t2, t3}) == 3
    for _ in range(2):
        assert np.array_equal(_product(rt, A1, W1, tag=t1), exact1.astype(np.float64))
        assert np.array_equal(_product(rt, A2, W2, tag=t2), exact2.astype(np.float64))
        assert np.array_equal(_product(rt, A3, W3, tag=t3), exact3.astype(np.float64))


def test_tagged_and_untagged_give_the_same_bits():
    from world import _hip

    rt = _rt()
    for pro, epi in ((0, 0), (2, 0), (1, 1), (0, 2)):
        A, P, pscale, W = R.pair_data(R.CENTRE, pro, epi, seed=9)
        plain = _product(rt, A, W, pro, P, pscale, epi)
        tagged = _product(rt, A, W, pro, P, pscale, epi, tag=_hip.table_tag(W))
        assert np.array_equal(_bits(plain), _bits(tagged)), (pro, epi)


# ---- f ---------------------------------------------------------------------------------------------------------------------
HEAD_D = (257, 1025, 2049)


@pytest.fixture(scope="module")
def spectra():
    from test_feature_tables_host import random_spectrum

    return {d: random_spectrum(9, d, 11 * d) for d in HEAD_D}


@pytest.mark.parametrize("nfilt", (40, 65, 80))
@pytest.mark.parametrize("d", HEAD_D)
def test_lfbank_head_at_other_sizes(spectra, d, nfilt):
    from test_feature_tables_host import ref_lfbank
    from world.features import lfbank_device

    rt = _rt()
    spec = spectra[d]
    got = lfbank_device(rt, rt.to_device(spec), nfilt=nfilt).cpu().numpy()
    ref = ref_lfbank(spec, nfilt=nfilt)
    assert got.shape == ref.shape == (9, nfilt)
    err = float(np.max(np.abs(got - ref)))
    print("lfbank D %d nfilt %d: worst |log energy - reference| %.3g" % (d, nfilt, err))
    assert err < 1e-11


@pytest.mark.parametrize("n0", (1, 13, 65))
@pytest.mark.parametrize("d", HEAD_D)
def test_cepstral_heads_at_other_sizes(spectra, d, n0):
    from test_feature_tables_host import ref_imcep_log, ref_mcep
    from world.features import imcep_device, mcep_device

    rt = _rt()
    spec = spectra[d]
    got = mcep_device(rt, rt.to_device(spec), n0=n0).cpu().numpy()
    ref = ref_mcep(spec, n0)
    assert got.shape == ref.shape == (9, n0)
    err = float(np.max(np.abs(got - ref)))
    fft_size = 2 * (d - 1)
    cep = 0.5 * np.random.RandomState(d + n0).standard_normal((9, n0))
    dec = imcep_device(rt, rt.to_device(cep), fft_size).cpu().numpy()
    dec_ref = np.exp(ref_imcep_log(cep, fft_size))
    assert dec.shape == dec_ref.shape == (9, d)
    rms = rel_rms(dec, dec_ref)
    print("D %d n0 %d: worst |cepstrum - reference| %.3g, decoded spectrum relative RMS %.3g" % (d, n0, err, rms))
    assert err < 1e-12
    assert rms < 1e-12


# ---- g ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,w", [(1, 1, 0), (1, 5, 3), (3, 39, 5), (7, 300, 2), (241, 32, 5), (4, 12, 9)])
def test_context_frames_against_the_slicing_definition(n, d, w):
    from world import _hip

    rt = _rt()
    X = np.random.RandomState(n + d + w).standard_normal((n, d))
    width = (2 * w + 1) * d
    raw = rt.torch.full((GUARD + n * width + GUARD,), SENTINEL, dtype=rt.torch.int64, device=rt.device)
    out_d = raw.view(rt.torch.float64)[GUARD:]
    _hip.check(rt.lib.wh_context_frames(rt.ctx, rt.stream(), rt.ptr(rt.to_device(X)), n, d, w, rt.ptr(out_d)))
    raw = raw.cpu().numpy()
    assert np.all(raw[:GUARD] == SENTINEL) and np.all(raw[-GUARD:] == SENTINEL)
    # world/main.py:360-365
    padded = np.r_[np.zeros((w, d)) + X[0], X, np.zeros((w, d)) + X[-1]]
    ref = np.array([padded[i:i + 2 * w + 1].flatten() for i in range(n)])
    assert np.array_equal(raw[GUARD:-GUARD].reshape(n, width), _bits(ref))
