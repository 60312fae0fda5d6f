"""GPU: the shared transform engine of csrc/wh_fft.h (fft_lds, fft_lds_from_regs, rfft_lds, irfft_lds), through
wh_fft_engine_probe, at every (N, NT, SNT, MAXR, direction) shape the kernels instantiate, against a long-double FFT
(tests/_fft_reference.py); and the twiddle block the transforms read, through wh_twiddle_read.

  a  dense Gaussian input, 37 transforms per shape: relative RMS error per transform <= 1e-15 sqrt(log2(Nc) / 9);
  b  unit impulses: every output is one product of stored twiddles, |got - ref| <= 2 * 2^-52 * passes;
  c  the real transforms at their edges (constant, alternating, a cosine on bin N/4; ignored imaginary parts; round trip);
  d  the header's claims about bits (wave-local = workgroup-wide 8-8-8, register-fed = LDS-fed, lockstep = alone);
  e  4096 transforms of 8 repeating inputs in one launch: every copy has the same bits, twice;
  f  the tables: every entry against long double, exact axes, conjugate symmetry, the passes' [k][r] copies.

Nc is the complex size of the transform (N for kinds 0 and 1, N / 2 for the real ones).  With WH_FFT_ACCURACY_OUT set to a
file name, test a appends its measured figures there, one line per shape (the way to write profiles/r13_fft_engine_accuracy.txt)."""
import os

import numpy as np
import pytest

import _fft_reference as R

pytestmark = pytest.mark.gpu

LD = R.LD


def _both(n, nt, snt, maxr=8):
    return [(0, n, nt, snt, maxr, 0), (0, n, nt, snt, maxr, 1)]


# (kind, n, nt, snt, maxr, inverse): WH_PROBE_SHAPES of csrc/wh_fft_probe.hip, read off the call sites
# (tests/test_fft_reference_host.py trips when one is added).  n is the template argument: twice the complex size for kinds 2, 3.
SHAPES = (
    # fft_lds: CheapTrick, forward and inverse
    _both(128, 128, 128) + _both(256, 128, 128) + _both(512, 128, 128) + _both(1024, 256, 256) + _both(2048, 256, 256)
    # the synthesis chains, two in lockstep and alone (D4C runs the forward ones of the second row too)
    + _both(256, 128, 256) + _both(512, 128, 256) + _both(1024, 256, 512) + _both(2048, 256, 512)
    + _both(256, 256, 256) + _both(512, 256, 256) + _both(1024, 512, 512) + _both(2048, 512, 512)
    # D4C at 4096 and 8192 points; the band filters' 4096-point inverse
    + [(0, 4096, 512, 512, 8, 0), (0, 8192, 512, 512, 8, 0), (0, 4096, 256, 256, 8, 1)]
    # what fft_lds_wave runs on its one wave; the workgroup-wide twin of the register-fed (1024, 128)
    + _both(512, 64, 64) + [(0, 1024, 128, 128, 8, 0)]
    # the radix-4 plans of tools/build_variants.py's d4c variants
    + [(0, 2048, 256, 256, 4, 0), (0, 4096, 512, 512, 4, 0), (0, 8192, 512, 512, 4, 0)]
    + [(2, 4096, 256, 256, 4, 0), (2, 8192, 512, 512, 4, 0), (2, 16384, 512, 512, 4, 0)]
    # fft_lds_wave: the chains of response_kernel<1024> (GT 128 and 256 in a 256-thread workgroup) and a one-wave workgroup
    + [(4, 512, nt, snt, 8, inv) for nt, snt in ((128, 256), (256, 256), (64, 64)) for inv in (0, 1)]
    # fft_lds_from_regs: D4C's windows
    + [(1, 1024, 128, 128, 8, 0), (1, 2048, 256, 256, 8, 0), (1, 4096, 512, 512, 8, 0)]
    # rfft_lds: SWIPE', CheapTrick, D4C, the love-train gate, the Requiem filter
    + [(2, n, nt, nt, 8, 0) for n, nt in ((64, 32), (128, 64), (256, 128), (512, 128), (512, 256), (1024, 64), (1024, 128),
                                          (1024, 256), (2048, 128), (2048, 256), (2048, 512), (4096, 256), (4096, 512),
                                          (8192, 256), (8192, 512), (16384, 256))]
    # irfft_lds (no caller today): CheapTrick's and D4C's rfft_lds shapes
    + [(3, n, nt, nt, 8, 1) for n, nt in ((256, 128), (512, 128), (1024, 128), (2048, 256), (4096, 256), (512, 256),
                                          (4096, 512), (8192, 512))]
)
assert len(set(SHAPES)) == len(SHAPES) == 71


def _id(s):
    return "k%d-n%d-nt%d-snt%d-r%d-%s" % (s[0], s[1], s[2], s[3], s[4], "inv" if s[5] else "fwd")


def _real(s):
    return s[0] in (2, 3)


def _nc(s):
    return s[1] // 2 if _real(s) else s[1]


def _dims(s):
    """doubles per transform: in, out"""
    kind, n = s[0], s[1]
    return {0: (2 * n, 2 * n), 1: (2 * n, 2 * n), 2: (n, n + 2), 3: (n + 2, n), 4: (2 * n, 2 * n)}[kind]


def _n_passes(s):
    nt = 64 if s[0] == 4 else s[2]  # (fft_lds_wave: the plan of one wave, whatever the group)
    return R.passes(_nc(s), nt, s[4]) + (1 if _real(s) else 0)  # (the real transforms' split butterfly is one more)


def _launch(s, x_d, out_d, count):
    from world import _hip

    rt = _hip.Runtime.get()
    kind, n, nt, snt, maxr, inv = s
    _hip.check(rt.lib.wh_fft_engine_probe(rt.ctx, rt.stream(), kind, n, nt, snt, maxr, inv, rt.ptr(x_d), rt.ptr(out_d), count))


def _probe(s, flat):
    """flat: (count, doubles in) float64 -> (count, doubles out) float64.  A shape the library refuses raises."""
    from world import _hip

    rt = _hip.Runtime.get()
    flat = np.ascontiguousarray(flat, dtype=np.float64)
    count = flat.shape[0]
    assert flat.shape[1] == _dims(s)[0]
    x_d = rt.to_device(flat.reshape(-1))
    out = rt.empty((count * _dims(s)[1],))
    _launch(s, x_d, out, count)
    return out.cpu().numpy().reshape(count, _dims(s)[1])


def _pack(re, im):
    return np.stack([np.asarray(re, dtype=np.float64), np.asarray(im, dtype=np.float64)], axis=-1).reshape(re.shape[0], -1)


def _unpack(flat):
    v = flat.reshape(flat.shape[0], -1, 2)
    return v[..., 0], v[..., 1]


def _to_input(s, re, im=None):
    return np.asarray(re, dtype=np.float64) if s[0] == 2 else _pack(re, im)


def _reference(s, re, im=None):
    """(re, im) in long double of what shape s computes on this input (im None for the real results of kind 3)."""
    if not _real(s):
        return R.fft((re, im), inverse=bool(s[5]))
    if s[0] == 2:
        return R.rfft(re)
    return R.irfft(re, im), None


def _result(s, flat):
    return (flat, None) if s[0] == 3 else _unpack(flat)


def _err2(got, ref):
    d = (got[0].astype(LD) - ref[0]) ** 2
    if ref[1] is not None:
        d = d + (got[1].astype(LD) - ref[1]) ** 2
    return d


def _rel_rms(got, ref):
    r2 = ref[0] ** 2 + (ref[1] ** 2 if ref[1] is not None else 0)
    return np.sqrt(np.sum(_err2(got, ref), axis=-1) / np.sum(r2, axis=-1)).astype(np.float64)


def _max_abs(got, ref):
    return float(np.sqrt(np.max(_err2(got, ref))))


def _bound_a(s):
    return 1e-15 * np.sqrt(np.log2(_nc(s)) / 9.0)


def _bound_b(s):
    return 2.0 * 2.0 ** -52 * _n_passes(s)


# ---- a. dense input ---------------------------------------------------------------------------------------------------
_dense_cache = {}


def _dense(s):
    """37 transforms of standard-normal data and their reference, per (kind, Nc, direction): shapes that differ in threads or
    radix only are judged on the same input."""
    key = (s[0] if _real(s) else 0, _nc(s), s[5])
    if key not in _dense_cache:
        rng = np.random.RandomState(1000 * key[0] + key[2] + 2 * int(np.log2(key[1])))
        n_in = {0: _nc(s), 2: 2 * _nc(s), 3: _nc(s) + 1}[key[0]]
        re = rng.standard_normal((37, n_in))
        im = None if key[0] == 2 else rng.standard_normal((37, n_in))  # (kind 3: bins 0 and N/2 carry imaginary parts too)
        ref = _reference((key[0],) + tuple(s[1:5]) + (key[2],), re, im)
        if key[0] == 0:
            f = np.fft.ifft(re + 1j * im, axis=1) * n_in if key[2] else np.fft.fft(re + 1j * im, axis=1)
            pocket = (f.real, f.imag)
        elif key[0] == 2:
            f = np.fft.rfft(re, axis=1)
            pocket = (f.real, f.imag)
        else:
            z = re + 1j * im
            z[:, 0] = z[:, 0].real
            z[:, -1] = z[:, -1].real
            pocket = (np.fft.irfft(z, axis=1) * (2 * _nc(s)), None)
        _dense_cache[key] = (re, im, ref, float(np.max(_rel_rms(pocket, ref))))
    return _dense_cache[key]


@pytest.mark.parametrize("s", SHAPES, ids=_id)
def test_a_dense_accuracy(s):
    re, im, ref, pocket = _dense(s)
    got = _result(s, _probe(s, _to_input(s, re, im)))
    rel = _rel_rms(got, ref)
    worst, bound = float(np.max(rel)), _bound_a(s)
    line = "%-34s passes %d  worst rel rms %.3e  bound %.3e  ratio %.3f  pocketfft %.3e  kernel/pocketfft %.2f" % (
        _id(s), _n_passes(s), worst, bound, worst / bound, pocket, worst / pocket)
    print(line)
    if os.environ.get("WH_FFT_ACCURACY_OUT"):
        with open(os.environ["WH_FFT_ACCURACY_OUT"], "a") as f:
            f.write(line + "\n")
    assert np.all(np.isfinite(rel)) and worst <= bound, line


# ---- b. impulses ------------------------------------------------------------------------------------------------------
def _positions(nc):
    if nc <= 512:
        return list(range(nc))
    pos = {0, 1, nc // 2, nc - 1}
    rng = np.random.RandomState(nc)
    for res in range(64):  # one position per residue class modulo 64: every swizzle row and every lane
        pos.add(int(res + 64 * rng.randint(nc // 64)))
    j = 1
    while 2 * j <= nc:  # one per octave [2^j, 2^(j+1))
        pos.add(int(j + rng.randint(j)))
        j *= 2
    return sorted(pos)


@pytest.mark.parametrize("s", SHAPES, ids=_id)
def test_b_impulses(s):
    kind, n, nc = s[0], s[1], _nc(s)
    pos = _positions(nc)
    if not _real(s):
        re = np.zeros((len(pos), nc))
        re[np.arange(len(pos)), pos] = 1.0
        im = np.zeros_like(re)
        cols = [R.dft_column(nc, p, inverse=bool(s[5])) for p in pos]
        scale = 1.0
    elif kind == 2:  # real samples 2q and 2q + 1: the real and the imaginary part of the packed element q
        pos = sorted({2 * q for q in pos} | {2 * q + 1 for q in pos})
        re = np.zeros((len(pos), n))
        re[np.arange(len(pos)), pos] = 1.0
        im = None
        cols = [tuple(v[:nc + 1] for v in R.dft_column(n, p)) for p in pos]
        scale = 1.0
    else:  # an impulse in frequency, bin k of the half spectrum: 2 cos(2 pi k j / n) (bins 0 and n/2: once)
        pos = sorted(set(pos) | {nc})
        re = np.zeros((len(pos), nc + 1))
        re[np.arange(len(pos)), pos] = 1.0
        im = np.zeros_like(re)
        cols = [((1 if p in (0, nc) else 2) * R.dft_column(n, p, inverse=True)[0], None) for p in pos]
        scale = 2.0  # (the outputs are twice as large, and so is a rounding error's absolute size)
    ref = (np.stack([c[0] for c in cols]), None if cols[0][1] is None else np.stack([c[1] for c in cols]))
    got = _result(s, _probe(s, _to_input(s, re, im)))
    err, bound = _max_abs(got, ref), scale * _bound_b(s)
    print("%-34s %d impulses, max |got - ref| %.3e, bound %.3e (%d passes)" % (_id(s), len(pos), err, bound, _n_passes(s)))
    assert err <= bound, (err, bound)


# ---- c. the real transforms at their edges ------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [s for s in SHAPES if s[0] == 2], ids=_id)
def test_c_real_edges(s):
    n = s[1]
    j = np.arange(n)
    x = np.stack([np.ones(n), 1.0 - 2.0 * (j & 1), np.array([1.0, 0.0, -1.0, 0.0])[j & 3]])  # constant, alternating, cos on bin n/4
    re, im = _unpack(_probe(s, x))
    assert np.all(im[:, 0] == 0.0) and np.all(im[:, n // 2] == 0.0)
    ref = np.zeros((3, n // 2 + 1))
    ref[0, 0], ref[1, n // 2], ref[2, n // 4] = n, n, n / 2
    # a sum of n samples of size 1: the bound of b on a unit impulse, times the peak it applies to
    for row, peak in ((0, n), (1, n), (2, n / 2)):
        err = max(float(np.max(np.abs(re[row] - ref[row]))), float(np.max(np.abs(im[row]))))
        assert err <= _bound_b(s) * peak, (row, err, _bound_b(s) * peak)
    # and the dense rows of a: bins 0 and n/2 of a real input are real, exactly
    dre, _, _, _ = _dense(s)
    _, dim = _unpack(_probe(s, dre))
    assert np.all(dim[:, 0] == 0.0) and np.all(dim[:, n // 2] == 0.0)


@pytest.mark.parametrize("s", [s for s in SHAPES if s[0] == 3], ids=_id)
def test_c_inverse_real_ignores_dc_and_nyquist_phase_and_round_trips(s):
    n = s[1]
    re, im, _, _ = _dense(s)
    clean = im.copy()
    clean[:, 0] = 0.0
    clean[:, -1] = 0.0
    assert np.any(im[:, 0] != 0.0) and np.any(im[:, -1] != 0.0)
    a, b = _probe(s, _pack(re, im)), _probe(s, _pack(re, clean))
    assert np.array_equal(a, b)  # "imaginary parts of the DC / Nyquist bins are ignored" (wh_fft.h)
    # irfft(rfft(x)) / n = x, through the forward shape of the same threads
    fwd = (2,) + tuple(s[1:5]) + (0,)
    assert fwd in SHAPES
    x = np.random.RandomState(n).standard_normal((37, n))
    back = _probe(s, _probe(fwd, x)) / n
    rel = _rel_rms((back, None), (x.astype(LD), None))
    print("%-34s round trip worst rel rms %.3e, bound %.3e" % (_id(s), float(np.max(rel)), _bound_a(s)))
    assert float(np.max(rel)) <= _bound_a(s), (float(np.max(rel)), _bound_a(s))


# ---- d. the header's claims about bits ----------------------------------------------------------------------------------
def _complex_input(n, count, seed):
    rng = np.random.RandomState(seed)
    return _pack(rng.standard_normal((count, n)), rng.standard_normal((count, n)))


@pytest.mark.parametrize("s", [s for s in SHAPES if s[0] == 4], ids=_id)
def test_d_wave_local_transform_has_the_bits_of_the_workgroup_wide_one(s):
    # "Where fft_lds<N, INV, GT> runs 8-8-8 (GT <= 128 at N = 512) this is the same plan, layout and twiddles: the same bits"
    x = _complex_input(512, 37, 5 + s[5])
    wave = _probe(s, x)
    for nt in (64, 128):
        assert np.array_equal(wave, _probe((0, 512, nt, nt, 8, s[5]), x)), nt


@pytest.fixture(scope="module")
def nocontract_report():
    import _variants as V

    V.ensure("nocontract")
    return V.run_script("_fft_variant_script.py", "nocontract", timeout=300)


@pytest.mark.parametrize("nt", [128, 64])
@pytest.mark.parametrize("inverse", [0, 1])
def test_d_new_probe_has_the_bits_of_wh_fft_probe(nocontract_report, nt, inverse):
    """fft_lds<512, INV, 128, 128> and fft_lds<512, INV, 64, 64> through the new probe against wh_fft_probe's wave-local
    result.  The two hooks sit in units with different contraction flags (wh_api.hip: off; wh_fft_probe.hip: fast, where a
    radix-8 butterfly's h * (x + y) fuses into the additions behind it — 12 v_fma_f64 in the forward 512-point kernel that
    the other build does not have), so in the shipped library they differ in the last bits although plan, layout and
    twiddles are the same.  Bits are compared where both are compiled alike (tests/_fft_variant_script.py); in the shipped
    library the two agree to rounding."""
    from world import _hip

    assert nocontract_report["lib"].endswith("libworld_hip_nocontract.so")
    r = nocontract_report["cases"]["nt%d-inv%d" % (nt, inverse)]
    assert r["equal"] and r["finite"], r
    rt = _hip.Runtime.get()
    x = _complex_input(512, 37, 5 + inverse)
    got = _probe((0, 512, nt, nt, 8, inverse), x)
    x_d = rt.to_device(x.reshape(-1))
    out = rt.empty((x.size,))
    gt, snt = (128, 256) if nt == 128 else (64, 64)
    _hip.check(rt.lib.wh_fft_probe(rt.ctx, rt.stream(), 512, gt, snt, inverse, rt.ptr(x_d), rt.ptr(out), 37))
    other = out.cpu().numpy().reshape(37, -1)
    rel = np.sqrt(np.sum((got - other) ** 2, axis=1) / np.sum(other ** 2, axis=1))
    assert float(np.max(rel)) <= 2e-15, float(np.max(rel))  # (each is held to 1e-15 from the reference: a above, test_hip_fft_wave.py)


@pytest.mark.parametrize("s", [s for s in SHAPES if s[0] == 1], ids=_id)
def test_d_register_fed_first_pass_has_the_bits_of_the_lds_fed_one(s):
    twin = (0,) + tuple(s[1:])
    assert twin in SHAPES
    x = _complex_input(s[1], 37, s[1])
    assert np.array_equal(_probe(s, x), _probe(twin, x))


@pytest.mark.parametrize("s", [s for s in SHAPES if s[0] == 0 and s[3] > s[2]], ids=_id)
def test_d_lockstep_buffers_have_the_bits_of_a_lone_one(s):
    alone = (s[0], s[1], s[2], s[2], s[4], s[5])
    assert alone in SHAPES
    x = _complex_input(s[1], 37, s[1] + s[5])  # 37: both buffer positions, and a last workgroup whose second buffer is idle
    assert np.array_equal(_probe(s, x), _probe(alone, x))


# ---- e. races -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", SHAPES, ids=_id)
def test_e_every_copy_of_an_input_has_the_same_bits(s):
    from world import _hip

    rt = _hip.Runtime.get()
    torch = rt.torch
    d_in, d_out = _dims(s)
    copies, distinct = 512, 8  # 4096 transforms: more workgroups than the card holds at once
    x8 = np.random.RandomState(s[1] + s[2]).standard_normal((distinct, d_in))
    x = rt.to_device(x8).repeat(copies, 1).contiguous()
    outs = []
    for _ in range(2):
        out = rt.empty((copies * distinct * d_out,))
        out.fill_(float("nan"))
        _launch(s, x, out, copies * distinct)
        outs.append(out.view(torch.int64).view(copies, distinct, d_out))
    differ = int((outs[0] != outs[0][0:1]).any(dim=2).sum().item())
    assert differ == 0, "%d of %d transforms differ from the first copy of their input" % (differ, copies * distinct)
    assert torch.equal(outs[0], outs[1])
    small = _probe(s, x8)  # and they are the bits of an 8-transform launch
    assert np.array_equal(outs[0][0].view(torch.float64).cpu().numpy(), small)
    assert np.all(np.isfinite(small))


# ---- f. the tables ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twiddle_block():
    import ctypes

    from world import _hip

    rt = _hip.Runtime.get()
    n = rt.lib.wh_twiddle_read(rt.ctx, None, 0)
    assert n == R.TWIDDLE_ENTRIES
    buf = np.full((n, 2), np.nan)
    _hip.check(rt.lib.wh_twiddle_read(rt.ctx, buf.ctypes.data_as(ctypes.c_void_p), n))
    assert rt.lib.wh_twiddle_read(rt.ctx, buf.ctypes.data_as(ctypes.c_void_p), n - 1) != 0
    return buf


def _sizes():
    n = 2
    while n <= R.MAX_TWIDDLE:
        yield n
        n *= 2


def test_f_every_table_entry_is_one_rounding_from_long_double(twiddle_block):
    tol = LD(2.0) ** -53 + LD(2.0) ** -63
    worst = LD(0)
    for n in _sizes():
        a = (LD(-2) * R.PI * np.arange(n).astype(LD)) / LD(n)  # the angle as the library's host code forms it
        tw = twiddle_block[n:2 * n].astype(LD)
        worst = max(worst, np.max(np.abs(tw[:, 0] - np.cos(a))), np.max(np.abs(tw[:, 1] - np.sin(a))))
        exact = R.twiddles(n)  # (and against the octant-folded evaluation, which does not round the angle near 2 pi)
        worst = max(worst, np.max(np.abs(tw[:, 0] - exact[0])), np.max(np.abs(tw[:, 1] - exact[1])))
    print("worst table entry: %.4e from long double (one rounding: %.4e)" % (float(worst), float(tol)))
    assert worst <= tol, (float(worst), float(tol))


def test_f_axis_entries_are_exact(twiddle_block):
    assert np.array_equal(twiddle_block[0:2], [[1.0, 0.0], [1.0, 0.0]])
    for n in _sizes():
        t = twiddle_block[n:2 * n]
        assert tuple(t[0]) == (1.0, 0.0) and tuple(t[n // 2]) == (-1.0, 0.0)
        if n >= 4:
            assert tuple(t[n // 4]) == (0.0, -1.0) and tuple(t[3 * n // 4]) == (0.0, 1.0)


def test_f_tables_are_conjugate_symmetric(twiddle_block):
    bad = {}
    for n in _sizes():
        t = twiddle_block[n:2 * n]
        k = np.arange(1, n)
        m = (t[n - k, 0] != t[k, 0]) | (t[n - k, 1] != -t[k, 1])
        if m.any():
            bad[n] = int(m.sum())
    assert not bad, "entries whose mirror is not their conjugate, per table size: %r" % bad


def test_f_pass_tables_are_copies_of_the_size_m_tables(twiddle_block):
    for r in (2, 4, 8):
        m = r
        while m <= R.MAX_FFT:
            off = R.ptw_offset(m, r)
            k = np.arange(m // r)[:, None]
            q = np.arange(1, r)[None, :]
            got = twiddle_block[off:off + (m // r) * (r - 1)].reshape(m // r, r - 1, 2)
            assert np.array_equal(got, twiddle_block[m + k * q]), (r, m)
            m *= 2
    assert R.ptw_offset(R.MAX_FFT, 8) + (R.MAX_FFT // 8) * 7 == R.TWIDDLE_ENTRIES  # the last table ends the block


def test_f_bad_arguments_are_refused():
    from world import _hip

    rt = _hip.Runtime.get()
    buf = rt.empty((4096,))
    p, st, probe = rt.ptr(buf), rt.stream(), rt.lib.wh_fft_engine_probe
    assert probe(rt.ctx, st, 0, 512, 128, 128, 8, 0, p, p, 1) == 0
    assert probe(None, st, 0, 512, 128, 128, 8, 0, p, p, 1) != 0          # null context
    assert probe(rt.ctx, st, 0, 512, 128, 128, 8, 0, None, p, 1) != 0     # null input
    assert probe(rt.ctx, st, 0, 512, 128, 128, 8, 0, p, None, 1) != 0     # null output
    assert probe(rt.ctx, st, 0, 512, 128, 128, 8, 0, p, p, -1) != 0       # negative count
    assert probe(rt.ctx, st, 0, 500, 128, 128, 8, 0, p, p, 1) != 0        # not a power of two
    assert probe(rt.ctx, st, 0, 512, 192, 192, 8, 0, p, p, 1) != 0        # a shape that is not built
    assert probe(rt.ctx, st, 0, 512, 128, 128, 2, 0, p, p, 1) != 0
    assert probe(rt.ctx, st, 4, 512, 128, 128, 8, 0, p, p, 1) != 0        # no such kind
    assert probe(rt.ctx, st, 2, 512, 128, 128, 8, 1, p, p, 1) != 0        # rfft_lds has one direction
    assert probe(rt.ctx, st, 0, 512, 128, 128, 8, 2, p, p, 1) != 0
    assert probe(rt.ctx, st, 0, 512, 128, 128, 8, 0, p, p, 0) == 0        # nothing to do
