"""The reference of tests/test_hip_fft_engine.py: a radix-2 decimation-in-time FFT in np.longdouble (plain NumPy, no GPU),
forward, inverse (unnormalised, like the kernels') and the real wrappers; and a restatement of wh::FftRadix
(csrc/wh_fft.h) that gives the passes of the plan the kernels run at (N, NT, MAXR).

An 80-bit x86 long double is assumed (eps 1.08e-19), as everywhere else in the suite that uses np.longdouble: the
reference's own error, ~2.5e-17 relative at N = 256, then lies a factor 40 under the 1e-15 the transforms are held to."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, (
    "tests/_fft_reference.py needs an extended-precision np.longdouble (x86 80-bit, eps 1.08e-19); here eps is %g: the "
    "reference would be no more precise than the FP64 transforms it judges" % np.finfo(LD).eps)

PI = LD("3.14159265358979323846264338327950288")  # 36 digits


def twiddles(n, sign=-1):
    """(cos, sin)(sign * 2 pi k / n), k < n, in long double.  The octants are folded onto [0, pi/4] first, so the axis
    entries are exact and every entry is as good as cosl / sinl of a small argument."""
    k = np.arange(n, dtype=np.int64)
    if n < 8:
        a = LD(sign) * LD(2) * PI * k.astype(LD) / LD(n)
        c, s = np.cos(a), np.sin(a)
        for arr in (c, s):
            arr[np.abs(arr) < LD(1e-15)] = LD(0)
        return c, s
    e = n // 8
    octant, r = k // e, k % e
    # angle = (octant * e + r) * 2 pi / n = octant * pi / 4 + r * 2 pi / n; odd octants count down from the next axis
    odd = (octant & 1) == 1
    rr = np.where(odd, e - r, r).astype(LD)
    a = LD(2) * PI * rr / LD(n)
    ca, sa = np.cos(a), np.sin(a)
    # cos / sin of the full angle theta = 2 pi k / n from the folded one
    q = ((octant + 1) // 2) % 4  # nearest axis: 0, pi/2, pi, 3 pi/2
    sgn = np.where(odd, LD(-1), LD(1))  # theta = axis + sgn * a
    cq = np.array([1, 0, -1, 0], dtype=LD)[q]
    sq = np.array([0, 1, 0, -1], dtype=LD)[q]
    c = cq * ca - sq * (sgn * sa)
    s = sq * ca + cq * (sgn * sa)
    return c, LD(sign) * s


def _bitrev(n):
    bits = n.bit_length() - 1
    idx = np.arange(n)
    rev = np.zeros(n, dtype=np.int64)
    for b in range(bits):
        rev |= ((idx >> b) & 1) << (bits - 1 - b)
    return rev


def fft(x, inverse=False):
    """Unnormalised DFT along the last axis, exp(-2 pi i j k / n) (inverse: +), of (re, im) given as a complex array or a
    pair of real arrays.  Returns a pair (re, im) of np.longdouble arrays."""
    if isinstance(x, tuple):
        re, im = (np.asarray(v, dtype=LD) for v in x)
    else:
        x = np.asarray(x)
        re, im = x.real.astype(LD), (x.imag.astype(LD) if np.iscomplexobj(x) else np.zeros(x.shape, dtype=LD))
    n = re.shape[-1]
    assert n >= 1 and n & (n - 1) == 0, n
    rev = _bitrev(n)
    re, im = re[..., rev].copy(), im[..., rev].copy()
    c, s = twiddles(n, +1 if inverse else -1) if n > 1 else (None, None)
    half = 1
    while half < n:
        step = n // (2 * half)
        wc, ws = c[::step][:half], s[::step][:half]
        shp = re.shape[:-1] + (n // (2 * half), 2, half)
        r4, i4 = re.reshape(shp), im.reshape(shp)
        ar, ai = r4[..., 0, :], i4[..., 0, :]
        br, bi = r4[..., 1, :], i4[..., 1, :]
        tr = br * wc - bi * ws
        ti = br * ws + bi * wc
        re = np.stack([ar + tr, ar - tr], axis=-2).reshape(re.shape)
        im = np.stack([ai + ti, ai - ti], axis=-2).reshape(im.shape)
        half *= 2
    return re, im


def dft_direct(x, inverse=False):
    """The O(n^2) sum itself, in long double: what fft() is checked against."""
    x = np.asarray(x)
    re, im = x.real.astype(LD), (x.imag.astype(LD) if np.iscomplexobj(x) else np.zeros(x.shape, dtype=LD))
    n = re.shape[-1]
    c, s = twiddles(n, +1 if inverse else -1)
    jk = (np.arange(n)[:, None] * np.arange(n)[None, :]) % n
    mc, ms = c[jk], s[jk]
    return re @ mc - im @ ms, re @ ms + im @ mc


def rfft(x):
    """n reals -> bins 0 .. n/2 of their DFT: (re, im)."""
    re, im = fft((np.asarray(x, dtype=LD), np.zeros(np.shape(x), dtype=LD)))
    n = re.shape[-1]
    return re[..., :n // 2 + 1], im[..., :n // 2 + 1]


def irfft(re, im):
    """n/2 + 1 bins -> the n real samples of the inverse DFT of their Hermitian extension, NOT divided by n (the imaginary
    parts of bins 0 and n/2 do not reach a real output and are ignored)."""
    re, im = np.asarray(re, dtype=LD).copy(), np.asarray(im, dtype=LD).copy()
    im[..., 0] = 0
    im[..., -1] = 0
    fr = np.concatenate([re, re[..., -2:0:-1]], axis=-1)
    fi = np.concatenate([im, -im[..., -2:0:-1]], axis=-1)
    return fft((fr, fi), inverse=True)[0]


def dft_column(n, p, inverse=False):
    """Column p of the DFT matrix: the transform of a unit impulse at p.  (re, im), exact to long-double rounding."""
    c, s = twiddles(n, +1 if inverse else -1)
    idx = (np.arange(n, dtype=np.int64) * int(p)) % n
    return c[idx], s[idx]


def plan(n, nt, maxr=8):
    """The radices of fft_lds<n, .., nt, .., maxr>'s passes: wh::FftRadix (csrc/wh_fft.h) restated."""
    out = []
    ns = 1
    while ns < n:
        r = 8 if (maxr >= 8 and ns * 8 <= n and n // 8 >= nt // 2) else (4 if ns * 4 <= n else 2)
        out.append(r)
        ns *= r
    assert ns == n, (n, nt, maxr, out)
    return out


def passes(n, nt, maxr=8):
    return len(plan(n, nt, maxr))


# fft_ptw_count / fft_ptw_offset and the sizes they are built from (csrc/wh_device.h), restated
MAX_FFT = 8192
MAX_TWIDDLE = 32768


def ptw_count(r):
    return (2 * MAX_FFT // r - 1) * (r - 1)


def ptw_offset(m, r):
    return 2 * MAX_TWIDDLE + (ptw_count(2) if r >= 4 else 0) + (ptw_count(4) if r >= 8 else 0) + (m // r - 1) * (r - 1)


TWIDDLE_ENTRIES = 2 * MAX_TWIDDLE + ptw_count(2) + ptw_count(4) + ptw_count(8)
