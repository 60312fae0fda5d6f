"""Inputs, runners and comparison shared by tests/test_hip_lsf.py, tests/_lsf_bounds_script.py and the host tests: seeded
autocorrelation rows, synthetic predictors built from chosen line spectral frequencies (expanded in mpmath, rounded once
to double) that need a given grid level, the degenerate rows, the reference result of every case (tests/_lsf_reference.py,
computed once per process and kept read-only), the three C entries called directly — inputs and outputs inside wider
tensors whose NaN guard bands must survive — and a bit-for-bit comparison."""
import collections
import functools

import numpy as np

import _lsf_reference as ref

ORDERS = (2, 4, 24, 40, 64)
FRAMES = (1, 63, 64, 65, 129, 257)
BINS = (129, 513, 1025, 2049)

Case = collections.namedtuple("Case", "name p frames k_bins pad seed")


@functools.lru_cache(maxsize=None)
def kernel_cases():
    """Every order with every frame count; the envelope's bins and the guard bands take turns."""
    cases = []
    for i, p in enumerate(ORDERS):
        for j, f in enumerate(FRAMES):
            n = i * len(FRAMES) + j
            cases.append(Case("p=%d F=%d K=%d%s" % (p, f, BINS[n % 4], " wide" if n % 2 else ""), p, f, BINS[n % 4],
                              3 if n % 2 else 0, n))
    return tuple(cases)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def spectra(frames, seed, k_bins=129):
    """Positive power spectra [frames][k_bins] with formant-like peaks, 60 dB of range."""
    rng = np.random.RandomState(1000 + seed)
    w = np.linspace(0, np.pi, k_bins)[None, :]
    s = np.full((frames, k_bins), 1e-3)
    for _ in range(5):
        centre = rng.uniform(0.1, 3.0, size=(frames, 1))
        width = rng.uniform(0.02, 0.3, size=(frames, 1))
        s = s + rng.uniform(0.1, 10.0, size=(frames, 1)) / (1.0 + ((w - centre) / width) ** 2)
    return _frozen(s * np.exp(rng.randn(frames, 1) * 3))


@functools.lru_cache(maxsize=None)
def reference(case):
    """{r, a, e, refl, bad, x, level, ex, env} of a case: each stage's reference on the reference's previous stage."""
    r = ref.autocorr(spectra(case.frames, case.seed), case.p)
    return stages(r, case.p, case.k_bins)


def stages(r, p, k_bins):
    a, e, refl, bad = ref.levinson(r, p)
    x, level = ref.lsf_from_lpc(a)
    ex = np.concatenate([e[:, None], x], axis=1)
    out = {"r": np.array(r), "a": a, "e": e, "refl": refl, "bad": bad, "x": x, "level": level, "ex": ex,
           "env": ref.envelope(e, x, k_bins)}
    _frozen(*out.values())
    return out


# ---- predictors that need a given grid level ---------------------------------------------------------------------------
def lpc_from_lsf(w):
    """The predictor a [p + 1] whose line spectral frequencies are w (radians, ascending, p even): P and Q expanded in
    mpmath at 60 digits, A = (P + Q) / 2 rounded once to double."""
    import mpmath

    with mpmath.workdps(60):
        def expand(first, angles):
            poly = [mpmath.mpf(1), mpmath.mpf(first)]
            for wi in angles:
                q = [mpmath.mpf(1), -2 * mpmath.cos(mpmath.mpf(float(wi))), mpmath.mpf(1)]
                new = [mpmath.mpf(0)] * (len(poly) + 2)
                for i, u in enumerate(poly):
                    for j, v in enumerate(q):
                        new[i + j] += u * v
                poly = new
            return poly

        pp, qq = expand(1, w[0::2]), expand(-1, w[1::2])
        return np.array([float((u + v) / 2) for u, v in zip(pp, qq)][:len(w) + 1])


def clustered_lsf(p, cell_level, straddle, half_gap, at=0.37):
    """p frequencies evenly spread, except that P's roots 2 i and 2 i + 2 and Q's root between them sit ``half_gap`` on
    either side of a point near ``at`` * pi: a point of level ``cell_level`` that no coarser level has (``straddle``) —
    that level separates the two, every coarser one sees them in one cell — or the middle of one of its cells."""
    w = np.pi * (np.arange(p) + 1.0) / (p + 1)
    i0 = 2 * int(round(at * p / 2))
    j = 2 * int(round(at * cell_level / 2)) + 1
    centre = np.pi * (j if straddle else j + 0.5) / cell_level
    w[i0], w[i0 + 1], w[i0 + 2] = centre - half_gap, centre + 0.3 * half_gap, centre + half_gap
    assert np.all(np.diff(w) > 0)
    return w


# (level the reference must need, or 0: exhausted and flagged) -> the frequencies; p = 24
REFINEMENT = ((256, None), (512, (512, True, 1.5e-3)), (1024, (1024, True, 1.0e-3)), (4096, (4096, True, 2.5e-4)),
              (0, (4096, False, 1.0e-4)))


@functools.lru_cache(maxsize=None)
def refinement_predictors(p=24):
    """(a [5][p + 1], the levels they are built for, the frequencies [5][p])."""
    ws = [np.pi * (np.arange(p) + 1.0) / (p + 1) if spec is None else clustered_lsf(p, *spec) for _, spec in REFINEMENT]
    a = np.stack([lpc_from_lsf(w) for w in ws])
    return _frozen(a, np.array([lv for lv, _ in REFINEMENT], dtype=np.int32), np.stack(ws))


@functools.lru_cache(maxsize=None)
def refinement_reference(p=24):
    a, _, _ = refinement_predictors(p)
    return _frozen(*ref.lsf_from_lpc(a))


# ---- degenerate rows next to clean ones ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def degenerate_rows(p=24):
    """(r [70][p + 1], the rows that are not clean): an all-zero row, a NaN in r[0], a NaN further on, r[0] < 0, +inf and
    a row whose error turns negative (|r[1]| > r[0]), among clean rows, across a wave's edge."""
    r = np.array(ref.autocorr(spectra(70, 77), p))
    odd = {3: "zero", 17: "nan0", 63: "nan5", 64: "neg", 65: "inf", 69: "indefinite"}
    r[3] = 0.0
    r[17, 0] = np.nan
    r[63, 5] = np.nan
    r[64, 0] = -r[64, 0]
    r[65, 0] = np.inf
    r[69, 1] = 1.5 * r[69, 0]
    return _frozen(r), odd


# ---- the entries, called directly -------------------------------------------------------------------------------------
def _wide_in(rt, a, pad):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if not pad:
        return rt.to_device(np.array(a))
    wide = np.full((a.shape[0], a.shape[1] + 2 * pad), np.nan)
    wide[:, pad:pad + a.shape[1]] = a
    return rt.to_device(wide)[:, pad:pad + a.shape[1]]


class _Out:
    """An output [rows][cols] inside a tensor of NaN with ``pad`` guard columns on either side."""

    def __init__(self, rt, rows, cols, pad, dtype=None):
        self.pad, self.cols = pad, cols
        self.wide = rt.torch.full((rows, cols + 2 * pad), float("nan"), dtype=dtype or rt.torch.float64, device=rt.device)
        self.view = self.wide[:, pad:pad + cols]
        self.ld = cols + 2 * pad

    def host(self):
        """(the rows, whether every guard column is still NaN)."""
        w = self.wide.cpu().numpy()
        guards = np.concatenate([w[:, :self.pad], w[:, self.pad + self.cols:]], axis=1)
        return w[:, self.pad:self.pad + self.cols].copy(), bool(np.all(np.isnan(guards)))


def run_levinson(rt, r, p, pad=0):
    """wh_lpc_levinson -> {a, e, refl, guards}."""
    from world import _hip

    r_d = _wide_in(rt, r, pad)
    f = int(r_d.shape[0])
    a, k = _Out(rt, f, p + 1, pad), _Out(rt, f, p, pad)
    e = rt.torch.full((f,), float("nan"), dtype=rt.torch.float64, device=rt.device)
    _hip.check(rt.lib.wh_lpc_levinson(rt.ctx, rt.stream(), rt.ptr(r_d), f, _hip.ld(r_d), p, rt.ptr(a.view), a.ld, rt.ptr(e),
                                      rt.ptr(k.view), k.ld))
    (ah, ga), (kh, gk) = a.host(), k.host()
    return {"a": ah, "e": e.cpu().numpy(), "refl": kh, "guards": ga and gk}


def run_lsf(rt, a, pad=0):
    """wh_lsf_from_lpc -> {x, level, guards}."""
    from world import _hip
    from world.lsf import grid_table

    a_d = _wide_in(rt, a, pad)
    f, p = int(a_d.shape[0]), int(a_d.shape[1]) - 1
    x = _Out(rt, f, p, pad)
    level = rt.torch.full((f,), -1, dtype=rt.torch.int32, device=rt.device)
    grid = grid_table()
    _hip.check(rt.lib.wh_lsf_from_lpc(rt.ctx, rt.stream(), rt.ptr(a_d), f, _hip.ld(a_d), p, _hip.f64p(grid), len(grid), rt.ptr(x.view),
                                      x.ld, rt.ptr(level)))
    xh, gx = x.host()
    return {"x": xh, "level": level.cpu().numpy(), "guards": gx}


def run_envelope(rt, ex, k_bins, pad=0):
    """wh_lsf_envelope -> {env, guards}."""
    from world import _hip
    from world.lsf import bin_table

    ex_d = _wide_in(rt, ex, pad)
    f, p = int(ex_d.shape[0]), int(ex_d.shape[1]) - 1
    out = _Out(rt, f, k_bins, pad)
    _hip.check(rt.lib.wh_lsf_envelope(rt.ctx, rt.stream(), rt.ptr(ex_d), f, _hip.ld(ex_d), p, _hip.f64p(bin_table(k_bins)), k_bins,
                                      rt.ptr(out.view), out.ld))
    eh, ge = out.host()
    return {"env": eh, "guards": ge}


def run(rt, case):
    """The three kernels of a case, each on the reference's input for it."""
    want = reference(case)
    got = run_levinson(rt, want["r"], case.p, case.pad)
    guards = got.pop("guards")
    two = run_lsf(rt, want["a"], case.pad)
    guards = guards and two.pop("guards")
    three = run_envelope(rt, want["ex"], case.k_bins, case.pad)
    guards = guards and three.pop("guards")
    got.update(two)
    got.update(three)
    got["guards"] = guards
    return got


KEYS = ("a", "e", "refl", "x", "level", "env")


def same_bits(x, y):
    """Equal shapes and equal values element by element, a NaN equal to a NaN."""
    x, y = np.asarray(x), np.asarray(y)
    if x.shape != y.shape:
        return False
    if x.dtype.kind != "f":
        return bool(np.array_equal(x, y))
    return bool(np.all((x == y) | (np.isnan(x) & np.isnan(y))))


def compare(got, want, keys=KEYS):
    """[] when every array equals the reference's bit for bit and the guard bands are intact."""
    bad = ["%s: %d of %d differ" % (k, int(np.sum(~((got[k] == want[k]) | ((got[k] != got[k]) & (want[k] != want[k]))))),
                                    got[k].size) for k in keys if not same_bits(got[k], want[k])]
    if not got.get("guards", True):
        bad.append("a guard band was written")
    return bad
