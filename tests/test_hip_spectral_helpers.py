"""GPU: the rectangular smoothing (BandWindow) and the low-band replica of CheapTrick and D4C on their own, in both forms —
the LDS form of csrc/wh_spectral.h through wh_spectral_probe at cheaptrick_kernel's (N, FT) pairs, the run-resident form of
csrc/wh_d4c_runs.h through wh_d4c_runs_probe at d4c_kernel's N — against tests/_spectral_reference.py (where the bounds used
here are derived).

  smoothing, bit for bit   integer spectra at dyadic fs / N, half-widths that are odd multiples of fs / N / 2 (f_lo = f_hi = 0)
                           and whole multiples of fs / N (both 0.5): every operation is exact, the output must equal integer
                           arithmetic — from the smallest window (b_hi == b_lo) to one wider than N / 2, through the mask;
  smoothing, within bound  half = f0 / 3 (CheapTrick), cf / 2 and cf / 4 (D4C), f0 = 40 ... 800 Hz at 22050 and 44100 Hz:
                           |error| of bin k0 + r <= (W + 2 r + 6) 2^-53 A on flat spectra, a 1/f^2 envelope, and a single bin
                           1e12 above its neighbours at every position of the half spectrum;
  replica                  an f0 grid per (fs, N) — on a bin and next to it, below one bin spacing, 40 ... 800 Hz, past one
                           wave's runs, around fs / 2 — with reach = f0 + fs / N and 1.2 f0: touched bins within
                           4 * 2^-53 (|slope dx| + |y_lo| + |p[k]|) of the long-double reference, untouched bins bit-identical
                           to the input, and the two forms bit-identical to each other wherever all nodes lie in the half
                           spectrum.

With WH_SPECTRAL_ACCURACY_OUT set to a file name, the bound tests append their measured figures there, one line per shape and
input: the largest error / bound and the largest error relative to the output itself (the way to write
profiles/r16_spectral_helpers_accuracy.txt)."""
import os

import numpy as np
import pytest

import _spectral_reference as S

pytestmark = pytest.mark.gpu

LD = S.LD
D4C_FT = S.D4C_FT  # ft_of(n), csrc/wh_d4c_types.h
# (form, n, ft): CheapTrick's pairs in the LDS form, D4C's in the run-resident one
SHAPES = [("lds", 256, 128), ("lds", 512, 128), ("lds", 1024, 128), ("lds", 2048, 256), ("lds", 4096, 256)] + [
    ("runs", n, D4C_FT[n]) for n in sorted(D4C_FT)]
DYADIC_FS = {256: 8000, 512: 8000, 1024: 16000, 2048: 16000, 4096: 48000, 8192: 96000}  # fs / n = 31.25, 15.625, 15.625, 7.8125, 11.71875 (twice)
REPLICA_FS = {256: 8000, 512: 16000, 1024: 16000, 2048: 16000, 4096: 48000, 8192: 96000}


def _id(s):
    return "%s-n%d-ft%d" % s


def _kr(s):
    return (s[1] // 2 + 1 + s[2] - 1) // s[2]


def _probe(s, which, fs, f0, rh, rows, rows_d=None):
    """rows (count, K) (or rows_d: the same, flat, on the device already), f0 / rh (count,) -> (count, K)"""
    from world import _hip

    rt = _hip.Runtime.get()
    form, n, ft = s
    k, count = n // 2 + 1, len(rh)
    if rows_d is None:
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        assert rows.shape == (count, k)
        rows_d = rt.to_device(rows.reshape(-1))
    assert rows_d.numel() == count * k and (f0 is None or len(f0) == count)
    x_d, rh_d = rows_d, rt.to_device(np.asarray(rh, dtype=np.float64))
    f0_d = rt.to_device(np.asarray(f0, dtype=np.float64)) if f0 is not None else None
    out = rt.empty((count * k,))
    out.fill_(float("nan"))
    if form == "lds":
        rc = rt.lib.wh_spectral_probe(rt.ctx, rt.stream(), n, ft, which, float(fs), rt.ptr(f0_d), rt.ptr(rh_d), rt.ptr(x_d),
                                      rt.ptr(out), count)
    else:
        rc = rt.lib.wh_d4c_runs_probe(rt.ctx, rt.stream(), n, which, float(fs), rt.ptr(f0_d), rt.ptr(rh_d), rt.ptr(x_d),
                                      rt.ptr(out), count)
    _hip.check(rc)
    return out.cpu().numpy().reshape(count, k)


def _upload(flat):
    from world import _hip

    return _hip.Runtime.get().to_device(flat)


def _record(line):
    print(line)
    if os.environ.get("WH_SPECTRAL_ACCURACY_OUT"):
        with open(os.environ["WH_SPECTRAL_ACCURACY_OUT"], "a") as f:
            f.write(line + "\n")


# ---- smoothing, bit for bit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", SHAPES, ids=_id)
def test_smoothing_of_integer_spectra_is_integer_arithmetic(s):
    _, n, _ = s
    fs = DYADIC_FS[n]
    df = fs / n
    spectra = np.random.RandomState(n).randint(0, 1000, (3, n // 2 + 1))
    spectra[2, 1:] = 0  # a lone DC bin: every window that holds it, holds it once (twice only through the wrap)
    halves = [j * df / 2 for j in (0, 1, 2, 3, 4, 7, 8, 41, 64, n // 2 + 3, n // 2 + 4)]
    widths = [S.band_constants(n, fs, h) for h in halves]
    assert widths[0][1] == widths[0][0] and widths[-1][1] - widths[-1][0] > n // 2
    rows = np.repeat(spectra, len(halves), axis=0).astype(np.float64)
    rh = np.tile(halves, len(spectra))
    got = _probe(s, 1, fs, None, rh, rows)
    bad = []
    for i in range(len(rows)):
        want = S.band_integer_reference(spectra[i // len(halves)], n, fs, rh[i])
        if not np.array_equal(got[i].view(np.int64), (want + 0.0).view(np.int64)):
            k = int(np.nonzero(got[i] != want)[0][0]) if np.any(got[i] != want) else -1
            bad.append((i // len(halves), rh[i] / df, k, got[i][k], want[k]))
    assert not bad, "(spectrum, half / df, first bin, got, want): %r" % bad[:6]


# ---- smoothing, within the derived bound ------------------------------------------------------------------------------------
F0S = (40.0, 47.0, 71.0, 150.0, 333.3, 800.0)
RATES = (22050, 44100)


def _halves(f0):
    cf = max(47.0, f0)
    return (f0 / 3, cf / 2, cf / 4)


def _spectrum(n, kind):
    rng = np.random.RandomState(n + len(kind))
    k = n // 2 + 1
    if kind == "flat":
        return rng.uniform(0.5, 1.5, k)
    return rng.chisquare(2, k) / (1.0 + np.arange(k)) ** 2  # "envelope": powers under 1/f^2


_ref_cache = {}


def _band_case(n, kind):
    """frames (fs, half), the spectrum, and per frame (v, consts, exactly rounded reference): shared by the two forms"""
    if (n, kind) not in _ref_cache:
        p = _spectrum(n, kind)
        frames = [(fs, h) for fs in RATES for f0 in F0S for h in _halves(f0)]
        per = []
        for fs, h in frames:
            v, consts = S.mirrored(p, n, fs), S.band_constants(n, fs, h)
            per.append((v, consts, S.band_reference(v, n, consts)))
        _ref_cache[(n, kind)] = (frames, p, per)
    return _ref_cache[(n, kind)]


@pytest.mark.parametrize("kind", ["flat", "envelope"])
@pytest.mark.parametrize("s", SHAPES, ids=_id)
def test_smoothing_error_within_the_bound(s, kind):
    _, n, _ = s
    frames, p, per = _band_case(n, kind)
    worst_ratio, worst_rel, bad = 0.0, 0.0, []
    for fs in RATES:  # (fs is an argument of the launch)
        idx = [i for i, fr in enumerate(frames) if fr[0] == fs]
        got = _probe(s, 1, fs, None, [frames[i][1] for i in idx], np.tile(p, (len(idx), 1)))
        for g, i in zip(got, idx):
            v, consts, ref = per[i]
            bound, _ = S.band_bound(v, n, consts, _kr(s))
            err = np.abs(g.astype(LD) - ref.astype(LD)).astype(np.float64)
            worst_ratio = max(worst_ratio, float(np.max(err / bound)))
            worst_rel = max(worst_rel, float(np.max(err / np.abs(ref))))
            if S.band_failures(g, ref, bound):
                bad.append((frames[i], S.band_failures(g, ref, bound)[:4]))
    _record("%-16s %-8s frames %4d  worst error / bound %.4f  worst error / |output| %.3e" % (
        _id(s), kind, len(frames), worst_ratio, worst_rel))
    assert not bad, bad[:4]


@pytest.mark.parametrize("fs", RATES)
@pytest.mark.parametrize("f0", F0S)
@pytest.mark.parametrize("s", SHAPES, ids=_id)
def test_smoothing_of_a_lone_peak_at_every_position(s, f0, fs):
    """One bin 1e12 above its flat neighbours, at EVERY bin of the half spectrum (K frames per launch), at the three
    half-widths of f0.  Where the window is narrower than a run the peak enters and leaves it inside the run, and u * peak
    stays in the running sum for the rest of that run.  The bound allows that (A holds the peak once the run has touched
    it); the figure that matters is the error relative to the output, recorded.
    Frame p differs from the flat frame only where a run has touched element p or N - p: everywhere else the flat frame's
    reference and bound hold, and there the reference is the flat one plus the peak's weight (S.band_add_peak)."""
    _, n, _ = s
    kr, k_bins, mask = _kr(s), n // 2 + 1, n - 1
    frames, base, per = _band_case(n, "flat")
    rows = np.tile(base, (k_bins, 1))
    rows[np.arange(k_bins), np.arange(k_bins)] = 1e12
    rows_d = _upload(rows.reshape(-1))  # once for the three launches
    del rows
    for half in _halves(f0):
        v, consts, base_ref = per[frames.index((fs, half))]
        base_bound, base_big = S.band_bound(v, n, consts, kr)
        factor = S.band_factor(n, consts, kr) * S.U
        start, length = S.run_touched(n, consts, kr)
        peak_v = 1e12 * (float(fs) / n)
        got = _probe(s, 1, fs, None, np.full(k_bins, half), None, rows_d=rows_d)
        finite = bool(np.all(np.isfinite(got)))
        err = np.abs(got - base_ref)  # (float64: exact where the two are close, and where they are not it is not small)
        rel = err / np.abs(base_ref)
        err /= base_bound
        for p in range(k_bins):
            where = sorted({p, (n - p) & mask})
            hit = np.zeros(k_bins, dtype=bool)
            for j in where:
                hit |= ((j - start) & mask) < length
            ks = np.nonzero(hit)[0]
            ref, big = base_ref[ks].astype(LD), base_big[ks].copy()
            for j in where:
                big += (peak_v - v[j]) * (((j - start[ks]) & mask) < length[ks])
                ref = S.band_add_peak(ref, ks, n, consts, j, LD(peak_v) - LD(v[j]))
            e = np.abs(got[p, ks].astype(LD) - ref)
            err[p, ks] = (e / (factor[ks] * big)).astype(np.float64)
            rel[p, ks] = (e / np.abs(ref)).astype(np.float64)
        worst_ratio, worst_rel = float(np.max(err)), float(np.max(rel))
        _record("%-16s peak     fs %5d f0 %5g half %7.3f  positions %4d  W %3d  worst error / bound %.4f  worst error / |output| %.3e" % (
            _id(s), fs, f0, half, k_bins, consts[1] - consts[0], worst_ratio, worst_rel))
        bad = np.argwhere(~(err <= 1.0))
        assert finite and len(bad) == 0, (half, "(position, bin):", bad[:6].tolist())


# ---- replica --------------------------------------------------------------------------------------------------------------
def _f0_grid(n, fs):
    df = fs / n
    # bins below 1.2 f0 that one wave's runs do not hold (d4c_kernel's run length; N = 256 is CheapTrick's alone: most of the half)
    past = 64 * ((n // 2 + 1 + D4C_FT[n] - 1) // D4C_FT[n]) + 8 if n in D4C_FT else n // 2 - 20
    on = 12 * df
    grid = [on, np.nextafter(on, 0.0), np.nextafter(on, np.inf), 0.4 * df, 40.0, 47.0, 150.0, 800.0,
            past * df / 1.2,                    # the one_wave == false branch of the run-resident form
            fs / 2 - 0.5 * df, fs / 2 + 0.5 * df]  # nodes above N / 2: the mirror branch of the LDS form
    assert past < n // 2
    return [float(f) for f in grid]


_replica_cache = {}


def _replica_case(n, fs):
    if (n, fs) not in _replica_cache:
        df = fs / n
        spectra = [_spectrum(n, "flat"), _spectrum(n, "envelope")]
        frames = [(f0, reach, j) for f0 in _f0_grid(n, fs) for reach in (f0 + df, 1.2 * f0) for j in range(len(spectra))]
        rows = np.stack([spectra[j] for _, _, j in frames])
        _replica_cache[(n, fs)] = (frames, rows, {})
    return _replica_cache[(n, fs)]


def _replica_fs(n):
    return (REPLICA_FS[n], 22050)


@pytest.mark.parametrize("s", SHAPES, ids=_id)
def test_replica_against_long_double(s):
    form, n, _ = s
    k_bins = n // 2 + 1
    cap = n if form == "lds" else k_bins
    for fs in _replica_fs(n):
        frames, rows, got_by_form = _replica_case(n, fs)
        got = _probe(s, 0, fs, [f[0] for f in frames], [f[1] for f in frames], rows)
        got_by_form[form] = got
        bad, seen = [], set()
        for i, (f0, reach, _) in enumerate(frames):
            ref, touched, bound = S.replica_reference(rows[i], n, fs, f0, reach, cap)
            nlow = S.replica_nlow(n, fs, reach, cap)
            seen.add(("untouched" if not touched.any() else "touched", "mirror" if nlow > k_bins else "half",
                      "waves" if nlow > 64 * _kr(s) else "wave"))
            fails = S.replica_failures(got[i], rows[i], ref, touched, bound)
            if fails:
                k = fails[0]
                bad.append((f0, reach, nlow, fails[:4], float(got[i][k]), float(ref[k]), float(bound[k])))
        assert not bad, "fs %d (f0, reach, nlow, bins, got, reference, bound): %r" % (fs, bad[:4])
        # the grid reaches what it is meant to reach: an untouched spectrum, several waves' worth of nodes, and (LDS form)
        # nodes above N / 2
        assert ("untouched", "half", "wave") in seen and any(t[2] == "waves" for t in seen)
        assert (form == "lds") == any(t[1] == "mirror" for t in seen)


@pytest.mark.parametrize("n", [512, 1024, 2048, 4096])
def test_replica_forms_have_each_others_bits(n):
    """low_band_replica and low_band_replica_runs are two implementations of one interpolation, compiled with the same
    contraction: wherever every node lies in the half spectrum (nlow <= K) they must agree bit for bit."""
    lds = [s for s in SHAPES if s[0] == "lds" and s[1] == n][0]
    runs = [s for s in SHAPES if s[0] == "runs" and s[1] == n][0]
    k_bins = n // 2 + 1
    for fs in _replica_fs(n):
        frames, rows, got_by_form = _replica_case(n, fs)
        for s in (lds, runs):
            if s[0] not in got_by_form:
                got_by_form[s[0]] = _probe(s, 0, fs, [f[0] for f in frames], [f[1] for f in frames], rows)
        compared, differ = 0, []
        for i, (f0, reach, _) in enumerate(frames):
            if S.replica_nlow(n, fs, reach, n) <= k_bins:
                compared += 1
                if not np.array_equal(got_by_form["lds"][i].view(np.int64), got_by_form["runs"][i].view(np.int64)):
                    differ.append((f0, reach, int(np.nonzero(got_by_form["lds"][i] != got_by_form["runs"][i])[0][0])))
        assert compared >= 30 and not differ, (fs, compared, differ[:6])


def test_bad_arguments_are_refused():
    from world import _hip

    rt = _hip.Runtime.get()
    x, o, v = rt.zeros((4097,)), rt.zeros((4097,)), rt.to_device(np.array([100.0]))
    px, po, pv, st = rt.ptr(x), rt.ptr(o), rt.ptr(v), rt.stream()
    lds, runs = rt.lib.wh_spectral_probe, rt.lib.wh_d4c_runs_probe
    assert lds(rt.ctx, st, 512, 128, 0, 16000.0, pv, pv, px, po, 1) == 0
    assert lds(rt.ctx, st, 512, 128, 1, 16000.0, None, pv, px, po, 1) == 0   # the smoothing takes no f0
    assert lds(rt.ctx, st, 512, 128, 0, 16000.0, None, pv, px, po, 1) != 0   # the replica does
    assert lds(None, st, 512, 128, 0, 16000.0, pv, pv, px, po, 1) != 0
    assert lds(rt.ctx, st, 512, 256, 0, 16000.0, pv, pv, px, po, 1) != 0     # not one of CheapTrick's pairs
    assert lds(rt.ctx, st, 8192, 256, 0, 16000.0, pv, pv, px, po, 1) != 0
    assert lds(rt.ctx, st, 512, 128, 2, 16000.0, pv, pv, px, po, 1) != 0
    assert lds(rt.ctx, st, 512, 128, 0, 0.0, pv, pv, px, po, 1) != 0
    assert lds(rt.ctx, st, 512, 128, 0, 16000.0, pv, pv, px, po, -1) != 0
    assert lds(rt.ctx, st, 512, 128, 0, 16000.0, pv, pv, px, po, 0) == 0
    assert runs(rt.ctx, st, 512, 0, 16000.0, pv, pv, px, po, 1) == 0
    assert runs(rt.ctx, st, 512, 1, 16000.0, None, pv, px, po, 1) == 0
    assert runs(rt.ctx, st, 512, 0, 16000.0, None, pv, px, po, 1) != 0
    assert runs(None, st, 512, 0, 16000.0, pv, pv, px, po, 1) != 0
    assert runs(rt.ctx, st, 256, 0, 16000.0, pv, pv, px, po, 1) != 0         # not a transform length of D4C
    assert runs(rt.ctx, st, 512, 2, 16000.0, pv, pv, px, po, 1) != 0
    assert runs(rt.ctx, st, 512, 0, 16000.0, pv, None, px, po, 1) != 0
    assert runs(rt.ctx, st, 512, 0, 16000.0, pv, pv, px, po, -1) != 0
    # a half-width outside [0, fs] is not walked: zeros come back
    big = rt.to_device(np.array([1e30]))
    one = rt.to_device(np.ones(257))
    res = rt.empty((257,))
    res.fill_(float("nan"))
    assert runs(rt.ctx, st, 512, 1, 16000.0, None, rt.ptr(big), rt.ptr(one), rt.ptr(res), 1) == 0
    assert np.array_equal(res.cpu().numpy(), np.zeros(257))
