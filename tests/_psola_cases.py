"""Inputs, runner and reference shared by tests/test_hip_psola.py, tests/test_psola_reference_host.py and
tests/_psola_bounds_script.py: the case list of wh_psola at the smallest shapes that reach every edge, the reference result
of every case (tests/_psola_reference.py, computed once per process and kept read-only) and the C entry called directly —
every output between guard values that must survive.

A case is one CALL: Params(grid, hop, tol, pmin, smin, norm) and a batch of utterances.  An utterance is
(signal, n, n_out, per_a, per_s, src):
    signal      tests/_wsola_cases.py's: noise, tone, silence, periodic (integers: exact score ties), half_silent, nan, inf;
                near_tie: 3.0 up to sample 32, then a block of eight values in [0.5, 1.5) repeated — with P = 64 the
                template of mark 0 is constant where it is not zero and the candidates d >= 0 read whole periods in
                rotated orders, so their scores are equal in real arithmetic and the winner is decided by the rounding
                of the sums in the contract's order (d < 0 reads the loud part and loses).
    n_out       an integer, or a float r: floor(r n + 0.5).
    per_a/per_s ("const", P); ("runs", (values, length)): runs of about `length` grid points, each one of the values;
                ("hostile", None): anything an int32 holds — negative, 1, above PMAX, the ends of the range — among legal ones.
    src         ("ratio", None): the uniform map for n_out / n; ("const", v); ("down", None): decreasing from n to 0;
                ("wild", None): anywhere from far in front of the utterance to far behind it, in no order;
                ("far", None): the same with +- 2^62 and the ends of the int64 range among them."""
import collections
import functools

import numpy as np

import _psola_reference as pref
import _wsola_cases as wc

Case = collections.namedtuple("Case", "name params utts seed")
P = pref.Params
PERIODS = (2, 3, 63, 64, 65, 255, 256, 257, 2048)
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
FIELDS = ("y", "marks", "periods", "smarks", "sel", "flip")
same_bits = wc.same_bits


def _frozen(a):
    a.setflags(write=False)
    return a


def _target(period, ratio):
    return int(min(max(2, np.floor(period / ratio + 0.5)), pref.PMAX))


@functools.lru_cache(maxsize=None)
def period_cases():
    """Every period, constant: pitch up and down at the recording's own timing, one noise and one tone."""
    cases = []
    for i, period in enumerate(PERIODS):
        n = min(max(40, 7 * period + 5), 7000)
        utts = (("noise", n, n, ("const", period), ("const", _target(period, 1.25)), ("ratio", None)),
                ("tone", n + 7, n + 7, ("const", period), ("const", _target(period, 0.8)), ("ratio", None)))
        cases.append(Case("P=%d" % period, P(16, 80, 50, 2, 1, 1), utts, i))
    runs = ("runs", (PERIODS + (0, 100, 100), 20))
    cases.append(Case("mixed periods", P(16, 80, 50, 2, 1, 1), (("tone", 9000, 9000, runs, runs, ("ratio", None)),
                                                               ("noise", 5000, 1.25, runs, ("const", 70), ("ratio", None))), 20))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def tol_cases():
    """2 D + 1 candidates on 256 threads: at P = 2048 D = min(tol, 512) — 1, 3, 255, 257 and 1025 candidates; at P = 65
    D = min(tol, 16)."""
    cases = [Case("P=2048 tol=%d" % tol, P(16, 80, tol, 2, 1, 1),
                  (("noise", 6300, 6300, ("const", 2048), ("const", 1800), ("ratio", None)),), 40 + i)
             for i, tol in enumerate((0, 1, 127, 128, 512))]
    cases += [Case("P=65 tol=%d" % tol, P(16, 80, tol, 2, 1, 1),
                   (("noise", 700, 700, ("const", 65), ("const", 52), ("ratio", None)), ("tone", 500, 500, ("const", 65), ("const", 80), ("ratio", None))), 50 + i)
              for i, tol in enumerate((15, 16, 17))]
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def edge_cases():
    speech = ("runs", ((0, 57, 64, 71, 80), 6))
    some = ("runs", ((0, 40, 63, 100, 100), 5))
    return (
        Case("G=1 U=1", P(1, 1, 8, 2, 1, 1), (("tone", 300, 300, ("runs", ((0, 31, 40), 60)), ("runs", ((0, 25, 50), 60)), ("ratio", None)),
                                             ("noise", 90, 1.25, ("const", 0), ("const", 0), ("ratio", None))), 100),
        Case("G=4096 U=2048", P(4096, 2048, 50, 2, 1, 1), (("tone", 9000, 9000, ("runs", ((0, 64, 100), 1)), ("runs", ((0, 80), 1)), ("ratio", None)),
                                                          ("noise", 4095, 4097, ("const", 0), ("const", 0), ("ratio", None))), 101),
        Case("pmin makes entries unvoiced", P(16, 80, 50, 60, 1, 1), (("tone", 2000, 2000, some, some, ("ratio", None)),), 102),
        Case("smin binds", P(16, 80, 50, 2, 90, 1), (("tone", 1500, 1500, ("const", 64), ("const", 50), ("ratio", None)),), 103),
        Case("norm 0", P(16, 80, 50, 2, 1, 0), (("tone", 1500, 1500, speech, ("const", 51), ("ratio", None)),
                                               ("noise", 700, 1.25, speech, speech, ("ratio", None))), 104),
        Case("empty, one sample, below P", P(16, 80, 50, 2, 1, 1), (("noise", 0, 0, ("const", 64), ("const", 64), ("ratio", None)),
                                                                    ("noise", 1, 1, ("const", 64), ("const", 64), ("ratio", None)),
                                                                    ("noise", 37, 37, ("const", 64), ("const", 50), ("ratio", None)),
                                                                    ("tone", 500, 500, ("const", 64), ("const", 50), ("ratio", None))), 105),
        Case("empty input, output asked for", P(16, 80, 50, 2, 1, 1), (("noise", 0, 200, ("const", 64), ("const", 64), ("wild", None)),
                                                                       ("tone", 300, 240, speech, speech, ("ratio", None))), 106),
        Case("output of one sample and of none", P(16, 80, 20, 2, 1, 1), (("noise", 300, 1, speech, speech, ("wild", None)),
                                                                          ("noise", 300, 0, speech, speech, ("ratio", None)),
                                                                          ("noise", 1, 0, ("const", 0), ("const", 0), ("ratio", None))), 107),
        Case("all voiced, all unvoiced", P(16, 80, 50, 2, 1, 1), (("tone", 1200, 1200, ("const", 57), ("const", 71), ("ratio", None)),
                                                                  ("noise", 1200, 1200, ("const", 0), ("const", 0), ("ratio", None))), 108),
        Case("stretch 0.5 and 2", P(16, 80, 50, 2, 1, 1), (("tone", 1600, 0.5, speech, speech, ("ratio", None)),
                                                           ("tone", 900, 2.0, speech, speech, ("ratio", None)),
                                                           ("noise", 600, 2.0, ("const", 0), ("const", 0), ("ratio", None))), 109),
        Case("constant src", P(16, 80, 50, 2, 1, 1), (("tone", 900, 700, speech, ("const", 60), ("const", 450)),
                                                      ("noise", 900, 500, ("const", 0), ("const", 0), ("const", 333))), 110),
        Case("src decreasing", P(16, 80, 50, 2, 1, 1), (("tone", 1200, 1200, speech, speech, ("down", None)),), 111),
        Case("src out of range", P(16, 80, 50, 2, 1, 1), (("tone", 900, 1100, speech, speech, ("wild", None)),
                                                          ("noise", 600, 2400, speech, speech, ("far", None))), 112),
        Case("src out of range G=1", P(1, 5, 3, 2, 1, 1), (("noise", 60, 50, ("const", 9), ("const", 7), ("far", None)),), 113),
        Case("hostile tracks", P(16, 80, 50, 2, 1, 1), (("tone", 2500, 2500, ("hostile", None), ("hostile", None), ("ratio", None)),
                                                        ("noise", 1500, 1.25, ("hostile", None), ("hostile", None), ("far", None))), 114),
        Case("target 2048 against analysis 20", P(16, 80, 50, 2, 1, 1), (("tone", 3000, 3000, ("const", 20), ("const", 2048), ("ratio", None)),), 115),
        Case("target 20 against analysis 2048", P(16, 80, 50, 2, 1, 1), (("tone", 6500, 3000, ("const", 2048), ("const", 20), ("ratio", None)),), 116),
        Case("target 2 against analysis 2048", P(16, 80, 0, 2, 1, 1), (("noise", 4500, 700, ("const", 2048), ("const", 2), ("ratio", None)),), 117),
        Case("digital silence", P(16, 80, 50, 2, 1, 1), (("silence", 900, 1.25, speech, speech, ("ratio", None)),
                                                         ("noise", 400, 1.25, speech, speech, ("ratio", None))), 118),
        Case("periodic integers: exact ties", P(16, 80, 7, 2, 1, 1), (("periodic", 400, 400, ("const", 20), ("const", 16), ("ratio", None)),
                                                                      ("periodic", 300, 1.25, ("const", 33), ("const", 40), ("ratio", None))), 119),
        Case("periodic integers: ties on two waves", P(16, 80, 200, 2, 1, 1), (("periodic", 2500, 2500, ("const", 400), ("const", 320), ("ratio", None)),), 120),
        Case("silence next to signal", P(16, 80, 50, 2, 1, 1), (("half_silent", 1200, 1.25, speech, speech, ("ratio", None)),
                                                                ("half_silent", 1200, 0.8, ("const", 64), ("const", 80), ("ratio", None))), 121),
        Case("ragged eight", P(16, 80, 50, 2, 1, 1), tuple(("tone" if k % 3 else "noise", 150 * k + 5, (1.0, 0.8, 1.25, 1.5, 0.5)[k % 5], speech,
                                                           ("const", 50 + 5 * k), ("ratio", None)) for k in range(8)), 122),
        Case("near ties: the order of the sums decides", P(16, 80, 8, 2, 1, 1), (("near_tie", 400, 400, ("const", 64), ("const", 51), ("ratio", None)),), 125),
    ) + tuple(Case("one %s" % {"nan": "NaN", "inf": "Inf"}[kind], P(16, 80, 50, 2, 1, 1),
                   (("tone", 900, 1.25, speech, speech, ("ratio", None)), (kind, 700, 0.8, speech, ("const", 60), ("ratio", None)),
                    ("noise", 500, 1.5, speech, speech, ("ratio", None))), 123 + i) for i, kind in enumerate(("nan", "inf")))


def all_cases():
    return period_cases() + tol_cases() + edge_cases()


def n_out_of(n, spec):
    return int(np.floor(spec * n + 0.5)) if isinstance(spec, float) else int(spec)


def signal(kind, n, rng):
    if kind != "near_tie":
        return wc.signal(kind, n, rng)
    x = np.tile(0.5 + np.random.RandomState(0).rand(8), n // 8 + 1)[:n]
    x[:32] = 3.0
    return x


def period_track(spec, count, rng):
    kind, arg = spec
    if kind == "const":
        return np.full(count, arg, dtype=np.int32)
    if kind == "runs":
        values, length = arg
        out = np.zeros(count, dtype=np.int32)
        k = 0
        while k < count:
            run = int(rng.randint(1, 2 * length + 1))
            out[k:k + run] = values[rng.randint(len(values))]
            k += run
        return out
    if kind == "hostile":
        pool = np.array([-1, -64, 0, 1, 2, 3, 57, 64, 80, 2048, 2049, 4096, 65536 + 64, INT32_MIN, INT32_MAX, INT32_MAX - 63], dtype=np.int64)
        return pool[rng.randint(len(pool), size=count)].astype(np.int32)
    raise ValueError(kind)


def source_track(spec, count, n, n_out, grid, rng):
    kind, arg = spec
    k = np.arange(count, dtype=np.float64)
    if kind == "ratio":
        return np.floor(k * grid * (float(n) / max(n_out, 1)) + 0.5).astype(np.int64)
    if kind == "const":
        return np.full(count, arg, dtype=np.int64)
    if kind == "down":
        return (n - np.floor(k * grid * (float(n) / max(n_out, 1)) + 0.5)).astype(np.int64)
    reach = 3000
    out = rng.randint(-reach, n + reach + 1, size=count).astype(np.int64)
    if kind == "far":
        far = [INT64_MIN, INT64_MAX, -2 ** 62, 2 ** 62, 2 ** 62 + 1, -2 ** 62 - 1, INT64_MAX - grid, INT64_MIN + grid, 2 ** 31, -2 ** 31 - 1]
        where = rng.permutation(count)[:len(far)]
        out[where] = np.array(far[:len(where)], dtype=np.int64)
    return out


@functools.lru_cache(maxsize=None)
def inputs(case):
    """{x, n_out, per_a, per_s, src}: tuples per utterance."""
    rng = np.random.RandomState(12000 + case.seed)
    grid = case.params.grid
    out = {k: [] for k in ("x", "n_out", "per_a", "per_s", "src")}
    for kind, n, n_out_spec, pa, ps, sr in case.utts:
        n_out = n_out_of(n, n_out_spec)
        out["x"].append(_frozen(signal(kind, n, rng)))
        out["n_out"].append(n_out)
        out["per_a"].append(_frozen(period_track(pa, n // grid + 1, rng)))
        out["per_s"].append(_frozen(period_track(ps, n_out // grid + 1, rng)))
        out["src"].append(_frozen(source_track(sr, n_out // grid + 1, n, n_out, grid, rng)))
    return {k: tuple(v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def reference(case):
    """The reference's {y, marks, periods, smarks, sel, flip} per utterance."""
    inp = inputs(case)
    out = []
    for u in range(len(case.utts)):
        r = pref.psola(inp["x"][u], inp["n_out"][u], inp["per_a"][u], inp["per_s"][u], inp["src"][u], case.params)
        out.append({k: _frozen(v) for k, v in r.items()})
    return tuple(out)


def call(rt, n_utt, x_off, y_off, pa_off, ps_off, mark_off, smark_off, params, x, per_a, per_s, src, y, marks=None, periods=None,
         n_marks=None, smarks=None, sel=None, flip=None, n_smarks=None):
    """The C entry with host arrays made from lists (pointers pass as they are); returns rc."""
    from world import _hip

    offs = [None if a is None else np.ascontiguousarray(a, dtype=np.int64) for a in (x_off, y_off, pa_off, ps_off, mark_off, smark_off)]
    return rt.lib.wh_psola(rt.ctx, rt.stream(), n_utt, *(None if a is None else _hip.i64p(a) for a in offs), *[int(v) for v in params],
                           x, per_a, per_s, src, y, marks, periods, n_marks, smarks, sel, flip, n_smarks)


GUARDS = {"y": -7.0, "marks": -777777777777, "periods": -77777, "smarks": -777777777771, "sel": -77771, "flip": 77, "n_marks": -7771,
          "n_smarks": -7773}
DTYPES = {"y": "float64", "marks": "int64", "periods": "int32", "smarks": "int64", "sel": "int32", "flip": "uint8", "n_marks": "int32",
          "n_smarks": "int32"}


def _cum(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def run(rt, case, only=None, xs=None, want_marks=True, slack=0):
    """wh_psola on a case -> {y, marks, periods, smarks, sel, flip: [per utterance], guards, rc}.  ``only``: that utterance
    alone, as a batch of one.  ``xs``: other signals than the case's.  ``want_marks`` False: every output but y is NULL.
    ``slack``: capacity beyond the least the contract asks for."""
    inp, p = inputs(case), case.params
    utts = list(range(len(case.utts))) if only is None else [only]
    xs = [(inp["x"] if xs is None else xs)[u] for u in utts]
    n_outs = [inp["n_out"][u] for u in utts]
    x_off, y_off = _cum([len(x) for x in xs]), _cum(n_outs)
    pa_off, ps_off = _cum([len(inp["per_a"][u]) for u in utts]), _cum([len(inp["per_s"][u]) for u in utts])
    mark_off = _cum([pref.mark_capacity(len(x), p) + slack for x in xs])
    smark_off = _cum([pref.smark_capacity(n, p) + slack for n in n_outs])
    torch = rt.torch

    def dev(parts, dtype):
        return torch.from_numpy(np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0), dtype=dtype)).to(rt.device)

    x_d = rt.to_device(np.concatenate(xs) if xs else np.zeros(0))
    pa_d, ps_d = dev([inp["per_a"][u] for u in utts], np.int32), dev([inp["per_s"][u] for u in utts], np.int32)
    src_d = dev([inp["src"][u] for u in utts], np.int64)
    sizes = {"y": int(y_off[-1]), "marks": int(mark_off[-1]), "periods": int(mark_off[-1]), "smarks": int(smark_off[-1]),
             "sel": int(smark_off[-1]), "flip": int(smark_off[-1]), "n_marks": len(xs), "n_smarks": len(xs)}
    w = {k: torch.full((sizes[k] + 2,), GUARDS[k], dtype=getattr(torch, DTYPES[k]), device=rt.device) for k in sizes}
    ptr = {k: (rt.ptr(w[k][1:]) if (want_marks or k == "y") else None) for k in sizes}
    rc = call(rt, len(xs), x_off, y_off, pa_off, ps_off, mark_off, smark_off, p, rt.ptr(x_d), rt.ptr(pa_d), rt.ptr(ps_d), rt.ptr(src_d),
              ptr["y"], ptr["marks"], ptr["periods"], ptr["n_marks"], ptr["smarks"], ptr["sel"], ptr["flip"], ptr["n_smarks"])
    h = {k: v.cpu().numpy() for k, v in w.items()}
    guards = all(h[k][0] == GUARDS[k] and h[k][-1] == GUARDS[k] for k in h)
    guards = guards and np.array_equal(x_d.cpu().numpy(), np.concatenate(xs) if xs else np.zeros(0), equal_nan=True)
    out = {"rc": rc, "y": [h["y"][1:-1][y_off[i]:y_off[i + 1]].copy() for i in range(len(xs))]}
    if not want_marks:
        guards = guards and all(bool(np.all(h[k] == GUARDS[k])) for k in h if k != "y")
        out["guards"] = bool(guards)
        return out
    na, ns = h["n_marks"][1:-1], h["n_smarks"][1:-1]
    for k in ("marks", "periods", "smarks", "sel", "flip"):
        off, cnt = (mark_off, na) if k in ("marks", "periods") else (smark_off, ns)
        out[k] = []
        for i in range(len(xs)):
            seg = h[k][1:-1][off[i]:off[i + 1]]
            c = int(min(max(cnt[i], 0), len(seg)))
            out[k].append(seg[:c].copy())
            guards = guards and 0 <= cnt[i] <= len(seg) and bool(np.all(seg[c:] == GUARDS[k]))  # (nothing beyond the count is written)
    out["guards"] = bool(guards)
    return out


def compare_case(case, got):
    """[what is wrong] of a run of the whole case."""
    if got["rc"] != 0:
        return ["rc %d" % got["rc"]]
    bad = []
    for u, want in enumerate(reference(case)):
        for k in FIELDS:
            if k not in got:
                continue
            g, w = got[k][u], want[k]
            ok = same_bits(g, w) if k == "y" else (g.dtype == w.dtype and g.tobytes() == w.tobytes())
            if not ok:
                diff = np.flatnonzero(g != w)[:1] if g.shape == w.shape else "the count (%d for %d)" % (len(g), len(w))
                bad.append("utterance %d: %s differs, first at %s" % (u, k, diff))
    if not got["guards"]:
        bad.append("a guard value was written or the input changed")
    return bad
